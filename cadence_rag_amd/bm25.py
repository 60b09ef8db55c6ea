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
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native

K1 = 1.2
B = 0.75
RANGE_ROWS = 16384        # row positions per workgroup of the scoring kernel (csrc/crag_kernels.h BM25_RANGE)
MAX_QUERIES = 64
MAX_TOKEN_BYTES = 255
TF_MAX = 65535            # tf is stored in 16 bits, saturating
WHERE_MAX = 65535         # token positions at or above this are not indexed (post_where is 16 bits wide)
SNIPPET_MAX_TERMS = 64    # term slots per query of the snippet windows (CRAG_BM25_SNIPPET_MAX_TERMS)
SNIPPET_STAGE = 1024      # positions of one (query, row) pair the snippet kernel keeps in LDS (BM25_SNIPPET_STAGE)
MAX_CLAUSES = 16          # constraint clauses per query (include/crag_dense.h CRAG_BM25_MAX_CLAUSES)
MAX_PHRASE_TERMS = 8      # terms per phrase (CRAG_BM25_MAX_PHRASE)
REQ_TERM, EXC_TERM, REQ_PHRASE, EXC_PHRASE, MATCH_NOTHING = 0, 1, 2, 3, 4   # clause kinds of the C ABI
# prefix and fuzzy items (include/crag_dense.h states the rule at crag_bm25_expand_host)
BM25_EXPAND_SLICE = 4096  # vocabulary terms per workgroup of the match kernel (csrc/crag_kernels.h BM25_EXPAND_SLICE)
MAX_EXPANSIONS = 64       # kept terms per expanding item (CRAG_BM25_MAX_EXPANSIONS)
MAX_EXPAND_ITEMS = 8      # expanding items per query (CRAG_BM25_MAX_EXPAND_ITEMS)
MAX_PATTERNS = 512        # patterns per call of the expand entry (CRAG_BM25_MAX_PATTERNS)
PREFIX, FUZZY1, FUZZY2 = 0, 1, 2            # kinds of an expanding item
OPTIONAL, REQUIRED, EXCLUDED = 0, 1, 2      # its roles
REQ_ANY, EXC_ANY = 0, 1                     # group kinds of crag_bm25_group_masks_host

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


class QuerySyntaxError(ValueError):
    """A query over the limits of the clause syntax (16 constraint clauses, 8 terms per phrase)."""


@dataclass(frozen=True)
class ParsedQuery:
    """A query string read by the rule of DESIGN.md 4.7c (include/crag_dense.h states it).
      clauses  the constraint clauses in item order: (kind, tokens), kind one of REQ_TERM, EXC_TERM (one token each),
               REQ_PHRASE, EXC_PHRASE (two to eight tokens, in phrase order)
      bag      the scored tokens in item order: those of every non-excluded item (optional and required terms, the
               members of required phrases)
      text     the non-excluded items' text joined by single spaces, operators and quotes removed: what a lane that
               applies no clauses (the trigram field) is given"""
    clauses: Tuple[Tuple[int, Tuple[str, ...]], ...]
    bag: Tuple[str, ...]
    text: str
    # the expanding items (parse_query(text, expand=True)) in item order: (role, kind, token), role one of
    # OPTIONAL, REQUIRED, EXCLUDED, kind one of PREFIX, FUZZY1, FUZZY2.  Their tokens are neither in `bag` nor in
    # `clauses`; `text` holds them, operator removed, unless excluded
    expansions: Tuple[Tuple[int, int, str], ...] = ()

    @property
    def has_constraints(self) -> bool:
        return bool(self.clauses)


# one item: an optional prefix where no text stands in front of it, then a quoted run (the closing quote may be missing)
# or a run without whitespace and quotes.  A lone prefix fails the first reading and is read as (tokenless) text
_ITEM = re.compile(r'(?:(?<!\S)([+-]))?(?:"([^"]*)"?|([^\s"]+))')


# an unquoted item that ends in one operator: `*`, `~`, `~1` or `~2` (the shortest text in front of it)
_OPERATOR = re.compile(r"(.*?)(\*|~[12]?)\Z", re.S)
_KIND_OF = {"*": PREFIX, "~": FUZZY1, "~1": FUZZY1, "~2": FUZZY2}


def parse_query(text: str, expand: bool = False) -> ParsedQuery:
    """Items are separated by whitespace outside double quotes; `"` opens a quoted item (it also ends an unquoted one),
    an unclosed quote runs to the end.  An item may carry one prefix, `+` or `-`, directly in front of it, at the start
    of the string or after whitespace; anywhere else the character is text.  Every item's text goes through `tokenize`;
    an item without tokens is dropped.  Unquoted: every token is a term of the item's kind (`+` required, `-` excluded,
    none optional).  Quoted: one token is a term, more are a phrase, required unless prefixed `-`.  Nothing else is
    syntax, unless `expand`: then an unquoted item may end in one operator -- `*` prefix, `~` / `~1` fuzzy with distance
    1, `~2` with distance 2 -- which counts only if the text in front of it tokenises to exactly one token (otherwise the
    whole item is read as without `expand`); such an item goes to `expansions`, not to `bag` or `clauses`.
    Raises QuerySyntaxError over 16 constraint clauses (required and excluded expanding items count), 8 terms in a
    phrase or 8 expanding items."""
    clauses: List[Tuple[int, Tuple[str, ...]]] = []
    bag: List[str] = []
    kept: List[str] = []
    expansions: List[Tuple[int, int, str]] = []
    constrained = 0             # required and excluded expanding items
    for prefix, inside, bare in _ITEM.findall(text or ""):
        quoted = not bare           # (a bare item is never empty; a quoted one may be)
        raw = inside if quoted else bare
        excluded = prefix == "-"
        op = _OPERATOR.match(raw) if expand and not quoted else None
        if op is not None:
            front = tokenize(op.group(1))
            if len(front) == 1:
                role = EXCLUDED if excluded else REQUIRED if prefix == "+" else OPTIONAL
                expansions.append((role, _KIND_OF[op.group(2)], front[0]))
                constrained += role != OPTIONAL
                if not excluded:
                    kept.append(op.group(1).strip())
                if len(expansions) > MAX_EXPAND_ITEMS:
                    raise QuerySyntaxError(f"a query holds at most {MAX_EXPAND_ITEMS} prefix or fuzzy items")
                if len(clauses) + constrained > MAX_CLAUSES:
                    raise QuerySyntaxError(f"a query holds at most {MAX_CLAUSES} constraint clauses")
                continue
        toks = tokenize(raw)
        if not toks:
            continue
        if quoted and len(toks) > 1:
            if len(toks) > MAX_PHRASE_TERMS:
                raise QuerySyntaxError(f"a phrase holds at most {MAX_PHRASE_TERMS} terms ({len(toks)} given)")
            clauses.append((EXC_PHRASE if excluded else REQ_PHRASE, tuple(toks)))
        elif excluded:
            clauses.extend((EXC_TERM, (tok,)) for tok in toks)
        elif quoted or prefix == "+":
            clauses.extend((REQ_TERM, (tok,)) for tok in toks)
        if not excluded:
            bag.extend(toks)
            kept.append(raw.strip())
        if len(clauses) + constrained > MAX_CLAUSES:
            raise QuerySyntaxError(f"a query holds at most {MAX_CLAUSES} constraint clauses")
    return ParsedQuery(tuple(clauses), tuple(bag), " ".join(kept), tuple(expansions))


class Bm25Index:
    """Vocabulary and per-row (term id, tf) pairs on the host, the inverted CSR on the device.

    Host (flat numpy arrays, the source of truth: `extend` appends to them and rebuilds the device side with numpy):
      vocab {token: term id}, ids handed out in order of first appearance
      row_ptr [N + 1] int64, row_terms [nnz] int32 (ascending inside a row), row_tf [nnz] int64, doc_len [N] int32
    Device: post_ptr [V + 1] int64, post_pos [nnz] int32 (row positions, ascending inside a term), post_tf [nnz] uint16,
      doc_len [N] int32, ids [N] int64.
    With positions=True (what phrase clauses need) the host also keeps every (row, term) pair's token
    positions, ascending -- pair_off [nnz + 1] int64 into pair_where uint16, in row order; positions at or above 65 535
    are not indexed -- and the device their permutation into posting order: post_off [nnz + 1] int64, post_where uint16:
    2 bytes per token and 8 per posting beside the 6 per posting of the lane."""

    def __init__(self, texts: Sequence[str], ids: Sequence[int], device, positions: bool = False) -> None:
        import torch
        self.device = torch.device(device) if not isinstance(device, torch.device) else device
        self.positions = bool(positions)
        self.pair_off = np.zeros(1, dtype=np.int64)
        self.pair_where = np.empty(0, dtype=np.uint16)
        self.vocab: Dict[str, int] = {}
        self.row_ptr = np.zeros(1, dtype=np.int64)
        self.row_terms = np.empty(0, dtype=np.int32)
        self.row_tf = np.empty(0, dtype=np.int64)
        self.doc_len = np.empty(0, dtype=np.int32)
        self.ids = np.empty(0, dtype=np.int64)
        self._ring = _native.UploadRing(self.device)
        self._buffers: dict = {}   # per (stream, name): grow-only device buffers (`_stream_buffer`)
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
        where: List[int] = []
        where_lens: List[int] = []
        for i, text in enumerate(texts):
            counts: Dict[int, int] = {}
            at: Dict[int, List[int]] = {}
            toks = tokenize(text)
            for p, tok in enumerate(toks):
                t = vocab.get(tok)
                if t is None:
                    t = vocab[tok] = len(vocab)
                counts[t] = counts.get(t, 0) + 1
                if self.positions and p < WHERE_MAX:
                    at.setdefault(t, []).append(p)
            row = sorted(counts.items())
            terms.extend(t for t, _ in row)
            tfs.extend(c for _, c in row)
            lens[i] = len(row)
            dls[i] = len(toks)
            if self.positions:
                for t, _ in row:
                    ps = at.get(t, ())
                    where.extend(ps)
                    where_lens.append(len(ps))
        if self.positions:
            self.pair_off = np.concatenate([self.pair_off, self.pair_off[-1] +
                                            np.cumsum(np.asarray(where_lens, dtype=np.int64))])
            self.pair_where = np.concatenate([self.pair_where, np.asarray(where, dtype=np.uint16)])
        self.row_ptr = np.concatenate([self.row_ptr, self.row_ptr[-1] + np.cumsum(lens)])
        self.row_terms = np.concatenate([self.row_terms, np.asarray(terms, dtype=np.int32)])
        self.row_tf = np.concatenate([self.row_tf, np.asarray(tfs, dtype=np.int64)])
        self.doc_len = np.concatenate([self.doc_len, dls])
        self.ids = np.concatenate([self.ids, new_ids])

    @classmethod
    def from_arrays(cls, row_ptr, row_terms, row_tf, n_terms: int, ids, device, vocab: Optional[Dict[str, int]] = None,
                    pair_off=None, pair_where=None) -> "Bm25Index":
        """An index over rows that are (term id, tf) pairs already (a synthetic corpus, or rows tokenised elsewhere):
        row_ptr [N + 1], row_terms ascending inside a row.  `vocab` maps tokens to term ids; without one the tokens of
        a query are the decimal term ids.  pair_off [nnz + 1] / pair_where: the token positions of every (row, term)
        pair, flat, in row order, ascending inside a pair (both or neither; with them the index has positions)."""
        self = cls([], [], device)
        if (pair_off is None) != (pair_where is None):
            raise ValueError("pair_off and pair_where come together")
        if pair_off is not None:
            self.positions = True
            self.pair_off = np.asarray(pair_off, dtype=np.int64).reshape(-1)
            self.pair_where = np.asarray(pair_where, dtype=np.uint16).reshape(-1)
            if self.pair_off.size != np.asarray(row_terms).size + 1 or self.pair_off[0] != 0 or \
                    np.any(np.diff(self.pair_off) < 0) or self.pair_off[-1] != self.pair_where.size:
                raise ValueError("pair_off must ascend from 0 to len(pair_where) with one entry per (row, term) pair + 1")
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

    def host_positions(self):
        """The token positions in posting order (the stable permutation of `host_csr`): post_off [nnz + 1] int64,
        post_where uint16 -- posting j holds its term at post_where[post_off[j] : post_off[j + 1]], ascending."""
        if not self.positions:
            raise ValueError("this index was built without positions")
        order = np.argsort(self.row_terms, kind="stable")
        lens = np.diff(self.pair_off)[order]
        post_off = np.zeros(order.size + 1, dtype=np.int64)
        np.cumsum(lens, out=post_off[1:])
        src = np.repeat(self.pair_off[:-1][order] - post_off[:-1], lens) + np.arange(post_off[-1], dtype=np.int64)
        return post_off, self.pair_where[src]

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
        self.d_post_off = self.d_post_where = None
        if self.positions:
            post_off, post_where = self.host_positions()
            self.d_post_off, self.d_post_where = dev(post_off), dev(post_where, np.int16)   # (bits of the uint16 values)
        self._buffers = {}
        self._dictionary = None      # (d_term_ptr, d_term_bytes): uploaded by the first `expand`, dropped here

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
        weights = _idf_weight(float(self.n), df, np.asarray(qtfs, dtype=np.float64))
        return q_ptr, term_ids, weights.astype(np.float32)   # fp64 up to here, rounded once

    # ---- device side -------------------------------------------------------------------------------------------
    def _slot(self, stream: int):
        """Next upload slot of the stream's ring of four."""
        return self._ring.slot(stream)

    def close(self) -> None:
        self._ring.close()

    def _stream_buffer(self, stream: int, name: str, min_bytes: int, dtype, alloc_bytes=None):
        """The stream's grow-only device buffer `name`, at least min_bytes large (`_upload` drops them all).  A buffer
        that has to be allocated takes max(min_bytes, alloc_bytes()) bytes, on `stream`."""
        buf = self._buffers.get((stream, name))
        if buf is None or buf.numel() * buf.element_size() < min_bytes:
            import torch

            from .fusion import _on_stream
            size = max(int(min_bytes), int(alloc_bytes()) if alloc_bytes else 0)
            with _on_stream(stream, self.device):
                buf = self._buffers[(stream, name)] = torch.empty(max(-(-size // dtype.itemsize), 1), dtype=dtype,
                                                                  device=self.device)
        return buf

    def search(self, query_texts: Sequence[str], k: int, row_mask=None, mask_stride: int = 0, stream: int = 0):
        """Top-k rows of every query by BM25 score (descending, equal scores by ascending id) among the rows that hold
        at least one query term and whose mask bit is set.  row_mask: packed bits per row position (uint8 CUDA tensor),
        shared (mask_stride 0) or per query.  Returns CUDA tensors ids int64 [nq, k] (-1 pad), scores fp32 [nq, k] (NaN
        pad), counts int32 [nq]; everything is enqueued on `stream` with one upload."""
        if len(query_texts) > MAX_QUERIES:
            raise ValueError("the BM25 lane takes at most 64 queries per call")
        return self.search_terms(*self.query_terms(query_texts), k, row_mask=row_mask, mask_stride=mask_stride,
                                 stream=stream)

    def clause_arrays(self, parsed_list: Sequence[ParsedQuery]):
        """The batch's constraint clauses as the host arrays of crag_bm25_clause_masks_host: c_ptr [nq + 1], c_kind,
        ct_ptr [n_clauses + 1], ct_terms (all int32).  An unknown token turns a required clause into kind 4 ("matches
        nothing") and drops an excluded one.  A phrase clause on an index without positions raises ValueError."""
        get = self.vocab.get
        per_query = []
        for parsed in parsed_list:
            items = []
            for kind, toks in parsed.clauses:
                if kind in (REQ_PHRASE, EXC_PHRASE) and not self.positions:
                    raise ValueError("a phrase clause needs an index built with positions=True")
                ids = [get(tok) for tok in toks]
                if any(t is None for t in ids):
                    if kind in (EXC_TERM, EXC_PHRASE):
                        continue
                    kind, ids = MATCH_NOTHING, []
                items.append((kind, ids))
            per_query.append(items)
        return _nested_csr(per_query)

    # ---- prefix and fuzzy items ----------------------------------------------------------------------
    def term_strings(self) -> List[str]:
        """The vocabulary's terms in term-id order (an index without a vocabulary: the decimal strings of the ids)."""
        if isinstance(self.vocab, _DecimalVocab):
            return [str(t) for t in range(len(self.vocab))]
        terms: List[Optional[str]] = [None] * len(self.vocab)
        for tok, t in self.vocab.items():
            terms[t] = tok
        if any(t is None for t in terms):
            raise ValueError("the vocabulary's term ids must be 0 .. len(vocab) - 1, each once")
        return terms

    def _device_dictionary(self):
        """d_term_ptr [V + 1] int64 and d_term_bytes, the UTF-8 bytes of the terms in term-id order: built and uploaded
        on first use, dropped by `_upload` (so `extend` stays correct)."""
        import torch
        if getattr(self, "_dictionary", None) is None:
            encoded = [t.encode("utf-8") for t in self.term_strings()]
            term_ptr = np.zeros(len(encoded) + 1, dtype=np.int64)
            np.cumsum(np.fromiter(map(len, encoded), dtype=np.int64, count=len(encoded)), out=term_ptr[1:])
            flat = np.frombuffer(b"".join(encoded) or b"\0", dtype=np.uint8)
            self._dictionary = (torch.from_numpy(term_ptr).to(self.device), torch.from_numpy(flat.copy()).to(self.device))
        return self._dictionary

    def expand(self, patterns: Sequence[Tuple[int, str]], stream: int = 0):
        """The vocabulary terms that the patterns stand for: patterns are (kind, token) with kind PREFIX, FUZZY1 or
        FUZZY2, at most 512 per call.  Returns per pattern (kept term ids int32, their distances int32, the number of all
        matches): the first 64 matches by distance ascending, df descending, term id ascending (crag_bm25_expand_host).
        One launch pair on `stream` and ONE stream synchronisation for the read-back."""
        import torch

        from .fusion import _on_stream
        patterns = list(patterns)
        if len(patterns) > MAX_PATTERNS:
            raise ValueError(f"the expand entry takes at most {MAX_PATTERNS} patterns per call")
        if not patterns:
            return []
        lib = _native.load()
        encoded = [tok.encode("utf-8") for _, tok in patterns]
        npat = len(patterns)
        pat_ptr = np.zeros(npat + 1, dtype=np.int32)
        np.cumsum([len(e) for e in encoded], out=pat_ptr[1:])
        pat_bytes = np.frombuffer(b"".join(encoded) or b"\0", dtype=np.uint8)
        pat_kind = np.asarray([kind for kind, _ in patterns], dtype=np.int32)
        d_term_ptr, d_term_bytes = self._device_dictionary()
        need = int(lib.crag_bm25_expand_scratch_bytes(self.n_terms, npat))
        scratch = self._stream_buffer(stream, "expand", need, torch.int64)
        with _on_stream(stream, self.device):
            # one buffer, one copy back: terms [np, 64] | dist [np, 64] | kept [np] | pad | total [np] int64
            words = 2 * npat * MAX_EXPANSIONS + (npat + 1) // 2 * 2
            out = torch.empty(words * 4 + npat * 8, dtype=torch.uint8, device=self.device)
        base = out.data_ptr()
        rc = lib.crag_bm25_expand_host(
            d_term_ptr.data_ptr(), d_term_bytes.data_ptr(), self.d_post_ptr.data_ptr(), self.n_terms,
            pat_ptr.ctypes.data, pat_bytes.ctypes.data, pat_kind.ctypes.data, npat, self._slot(stream),
            scratch.data_ptr(), scratch.numel() * 8, base, base + npat * MAX_EXPANSIONS * 4,
            base + 2 * npat * MAX_EXPANSIONS * 4, base + words * 4, ctypes.c_void_p(stream))
        _native.check(rc, "crag_bm25_expand_host")
        with _on_stream(stream, self.device):
            host = out.cpu().numpy()    # (synchronises the stream)
        i32 = host[:words * 4].view(np.int32)
        terms = i32[:npat * MAX_EXPANSIONS].reshape(npat, MAX_EXPANSIONS)
        dist = i32[npat * MAX_EXPANSIONS:2 * npat * MAX_EXPANSIONS].reshape(npat, MAX_EXPANSIONS)
        kept = i32[2 * npat * MAX_EXPANSIONS:2 * npat * MAX_EXPANSIONS + npat]
        total = host[words * 4:].view(np.int64)
        return [(terms[i, :kept[i]].copy(), dist[i, :kept[i]].copy(), int(total[i])) for i in range(npat)]

    def expanded_terms(self, parsed_list: Sequence[ParsedQuery], expansions):
        """The weights of DESIGN.md 4.7d for a batch: `expansions` holds the result of `expand` for every expanding item
        of the batch, in query order and item order.  Returns the arrays of `query_terms` (q_ptr, term ids ascending
        inside a query, fp32 weights): today's qtf * idf * (k1 + 1) for a term of the plain bag, plus base_j * 2^-d for
        every non-excluded item j that keeps the term, in item order, fp64, rounded once."""
        q_ptr = np.zeros(len(parsed_list) + 1, dtype=np.int32)
        terms: List[int] = []
        weights: List[float] = []
        get = self.vocab.get
        n = float(self.n)
        at = 0
        for q, parsed in enumerate(parsed_list):
            qtf: Dict[int, int] = {}
            for tok in parsed.bag:
                t = get(tok)
                if t is not None:
                    qtf[t] = qtf.get(t, 0) + 1
            w: Dict[int, float] = {}
            for t, c in qtf.items():
                w[t] = float(_idf_weight(n, float(self.df[t]), float(c)))
            for role, _, _ in parsed.expansions:
                ids, dist, _ = expansions[at]
                at += 1
                if role == EXCLUDED or len(ids) == 0:
                    continue
                base = float(_idf_weight(n, float(self.df[ids].max())))
                for t, d in zip(ids.tolist(), dist.tolist()):
                    w[t] = w.get(t, 0.0) + base * 2.0 ** (-d)
            ordered = sorted(w)
            terms.extend(ordered)
            weights.extend(w[t] for t in ordered)
            q_ptr[q + 1] = len(terms)
        return q_ptr, np.asarray(terms, dtype=np.int32), np.asarray(weights, dtype=np.float64).astype(np.float32)

    @staticmethod
    def group_arrays(parsed_list: Sequence[ParsedQuery], expansions):
        """The required and excluded expanding items of a batch as the host arrays of crag_bm25_group_masks_host: g_ptr
        [nq + 1], g_kind, gt_ptr [n_groups + 1], gt_terms (all int32).  A required item without a match stays as an empty
        group (it matches nothing); an excluded one without a match is dropped."""
        per_query = []
        at = 0
        for parsed in parsed_list:
            items = []
            for role, _, _ in parsed.expansions:
                ids = expansions[at][0]
                at += 1
                if role == OPTIONAL or (role == EXCLUDED and len(ids) == 0):
                    continue
                items.append((REQ_ANY if role == REQUIRED else EXC_ANY, ids.tolist()))
            per_query.append(items)
        return _nested_csr(per_query)

    def search_query(self, query_texts: Sequence[str], k: int, row_mask=None, mask_stride: int = 0, stream: int = 0,
                     expand: bool = False):
        """`search` for queries in the clause syntax of `parse_query` (+required, -excluded, "quoted phrase"): the rows
        that pass every clause and the mask, ranked by the BM25 score of the query's non-excluded tokens.  A batch
        without any constraint IS `search` (same calls, same bits).  Otherwise one launch turns the clauses into a row
        mask per query (crag_bm25_clause_masks_host, into a buffer this stream keeps) and `search_terms` scores under it.
        expand: also read `*`, `~`, `~1`, `~2` behind a token.  A batch without such an item makes exactly
        the calls above.  Otherwise: `expand` (one stream synchronisation), the required and excluded items as any-of row
        masks (crag_bm25_group_masks_host), the clause masks on top of them when plain clauses exist, and `search_terms`
        with the rule's weights.
        Raises QuerySyntaxError for a query over the limits, ValueError for a phrase on an index without positions."""
        if len(query_texts) > MAX_QUERIES:
            raise ValueError("the BM25 lane takes at most 64 queries per call")
        parsed = [parse_query(text, expand=expand) for text in query_texts]
        if any(p.expansions for p in parsed):
            return self._search_expanded(parsed, k, row_mask, mask_stride, stream)
        if not any(p.has_constraints for p in parsed):
            return self.search(query_texts, k, row_mask=row_mask, mask_stride=mask_stride, stream=stream)
        clauses = self.clause_arrays(parsed)
        bags = self.query_terms([" ".join(p.bag) for p in parsed])   # (tokens are alphanumeric runs: they re-tokenise as
        if self.n == 0:                                              #  themselves)
            return self.search_terms(*bags, k, stream=stream)
        stride = (self.n + 31) // 32 * 4
        buf = self._clause_masks(clauses, len(parsed), row_mask, mask_stride, stride, stream)
        return self.search_terms(*bags, k, row_mask=buf, mask_stride=stride, stream=stream)

    def _mask_launch(self, entry_name, extra_pointers, ptr, kind, t_ptr, terms, nq, in_mask, in_stride, buf, stride,
                     stream) -> None:
        """One launch of a mask entry (crag_bm25_clause_masks_host, crag_bm25_group_masks_host): the arrays of
        `clause_arrays` / `group_arrays` under `in_mask` into `buf`.  extra_pointers: what the entry takes between the
        postings and n_rows."""
        rc = getattr(_native.load(), entry_name)(
            self.d_post_ptr.data_ptr(), self.d_post_pos.data_ptr(), *extra_pointers, self.n, self.n_terms,
            ptr.ctypes.data, kind.ctypes.data if kind.size else None, t_ptr.ctypes.data,
            terms.ctypes.data if terms.size else None, nq, None if in_mask is None else in_mask.data_ptr(),
            int(in_stride), self._slot(stream), buf.data_ptr(), stride, ctypes.c_void_p(stream))
        _native.check(rc, entry_name)

    def _clause_launch(self, c_ptr, c_kind, ct_ptr, ct_terms, nq, in_mask, in_stride, buf, stride, stream) -> None:
        where = tuple(None if t is None else t.data_ptr() for t in (self.d_post_off, self.d_post_where))
        self._mask_launch("crag_bm25_clause_masks_host", where, c_ptr, c_kind, ct_ptr, ct_terms, nq, in_mask, in_stride,
                          buf, stride, stream)

    def _clause_masks(self, clauses, nq, in_mask, in_stride, stride, stream):
        """The clause masks of a batch under `in_mask`, in the buffer this stream keeps for a full batch of them."""
        import torch
        buf = self._stream_buffer(stream, "clause_masks", MAX_QUERIES * stride, torch.uint8)
        self._clause_launch(*clauses, nq, in_mask, in_stride, buf, stride, stream)
        return buf

    def _search_expanded(self, parsed, k, row_mask, mask_stride, stream):
        """`search_query` for a batch with expanding items: expand -> group masks -> clause masks -> search_terms."""
        expansions = self.expand([(kind, tok) for p in parsed for _, kind, tok in p.expansions], stream=stream)
        bags = self.expanded_terms(parsed, expansions)
        clauses = self.clause_arrays(parsed) if any(p.has_constraints for p in parsed) else None
        if self.n == 0:
            return self.search_terms(*bags, k, stream=stream)
        groups = self.group_arrays(parsed, expansions)
        stride = (self.n + 31) // 32 * 4
        mask, in_stride = row_mask, int(mask_stride)
        if groups[1].size:
            import torch
            buf = self._stream_buffer(stream, "group_masks", MAX_QUERIES * stride, torch.uint8)
            self._mask_launch("crag_bm25_group_masks_host", (), *groups, len(parsed), mask, in_stride, buf, stride, stream)
            mask, in_stride = buf, stride
        if clauses is not None:     # (the group mask is the clause launch's input: in and out must not overlap)
            mask, in_stride = self._clause_masks(clauses, len(parsed), mask, in_stride, stride, stream), stride
        return self.search_terms(*bags, k, row_mask=mask, mask_stride=in_stride, stream=stream)

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
        # the partial top-k lists: sized for a full batch at this k, so that a stream allocates once
        scratch = self._stream_buffer(stream, "topk", need, torch.int64,
                                      lambda: lib.crag_bm25_scratch_bytes(self.n, MAX_QUERIES, k))
        with _on_stream(stream, self.device):
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

    # ---- query-aware snippet windows ---------------------------------------------------------------
    def snippet_terms(self, query_texts: Sequence[str]):
        """The term slots of `snippet_windows`: the bag reading of every query -- `query_terms` of the non-excluded
        tokens of the clause syntax (required terms and phrase members count as plain terms; a query over the syntax's
        limits is tokenised as it stands) --, cut to the SNIPPET_MAX_TERMS heaviest slots of a query, equal weights by
        the lower term id, the kept slots back in ascending term-id order."""
        bags = []
        for text in query_texts:
            try:
                bags.append(" ".join(parse_query(text).bag))
            except QuerySyntaxError:
                bags.append(text)
        return heaviest_slots(*self.query_terms(bags), SNIPPET_MAX_TERMS)

    def snippet_windows(self, query_texts: Sequence[str], row_ids_per_query: Sequence[Sequence[int]], window: int,
                        stream: int = 0):
        """For every query and every row id listed for it: the window of `window` tokens of the row that holds the most of
        the query, by the rule of crag_bm25_snippets_host (include/crag_dense.h).  Returns CUDA tensors laid out along
        r_ptr, the running count of the lists: start int32 (-1: no query term in the row), last int32, score fp32, covered
        int64 (the bits of the rule's uint64: bit j is slot j of `snippet_terms`).  One upload and one launch on `stream`.
        Raises ValueError for an id the index does not hold and for an index built without positions."""
        if not self.positions:
            raise ValueError("snippet windows need an index built with positions=True")
        if len(query_texts) != len(row_ids_per_query):
            raise ValueError("one list of row ids per query")
        r_ptr = np.zeros(len(query_texts) + 1, dtype=np.int32)
        np.cumsum([len(ids) for ids in row_ids_per_query], out=r_ptr[1:])
        flat = np.asarray([rid for ids in row_ids_per_query for rid in ids], dtype=np.int64)
        rows = np.searchsorted(self.ids, flat)
        if flat.size and (np.any(rows >= self.ids.size) or np.any(self.ids[np.minimum(rows, self.ids.size - 1)] != flat)):
            raise ValueError("snippet_windows: a row id the index does not hold")
        return self.snippet_windows_terms(*self.snippet_terms(query_texts), r_ptr, rows.astype(np.int32), window,
                                          stream=stream)

    def snippet_windows_terms(self, q_ptr, terms, weights, r_ptr, rows, window: int, stream: int = 0):
        """`snippet_windows` for queries that are term slots already (the arrays of `query_terms`, at most
        SNIPPET_MAX_TERMS slots per query) and rows that are row positions: r_ptr [nq + 1] int32, rows int32."""
        import torch

        from .fusion import _on_stream
        if not self.positions:
            raise ValueError("snippet windows need an index built with positions=True")
        nq = len(q_ptr) - 1
        if nq > MAX_QUERIES or len(r_ptr) != nq + 1:
            raise ValueError("snippet windows take at most 64 queries per call, with one r_ptr entry per query + 1")
        q_ptr, r_ptr = np.ascontiguousarray(q_ptr, dtype=np.int32), np.ascontiguousarray(r_ptr, dtype=np.int32)
        terms, rows = np.ascontiguousarray(terms, dtype=np.int32), np.ascontiguousarray(rows, dtype=np.int32)
        weights = np.ascontiguousarray(weights, dtype=np.float32)
        npairs = int(r_ptr[-1]) if nq else 0
        with _on_stream(stream, self.device):
            start = torch.empty(npairs, dtype=torch.int32, device=self.device)
            last = torch.empty(npairs, dtype=torch.int32, device=self.device)
            score = torch.empty(npairs, dtype=torch.float32, device=self.device)
            covered = torch.empty(npairs, dtype=torch.int64, device=self.device)
        if nq == 0:
            return start, last, score, covered
        rc = _native.load().crag_bm25_snippets_host(
            self.d_post_ptr.data_ptr(), self.d_post_pos.data_ptr(), self.d_post_off.data_ptr(),
            self.d_post_where.data_ptr(), self.n, self.n_terms, q_ptr.ctypes.data,
            terms.ctypes.data if terms.size else None, weights.ctypes.data if weights.size else None, r_ptr.ctypes.data,
            rows.ctypes.data if rows.size else None, nq, int(window), self._slot(stream),
            start.data_ptr(), last.data_ptr(), score.data_ptr(), covered.data_ptr(), ctypes.c_void_p(stream))
        _native.check(rc, "crag_bm25_snippets_host")
        return start, last, score, covered


def _idf_weight(n, df, qtf=1.0):
    """qtf * idf(df) * (k1 + 1) in fp64, in this order of operations: numpy arrays or Python floats (numpy's vector
    and scalar log are not promised to agree in the last bit, so a caller stays with the kind it always used)."""
    return qtf * np.log(1.0 + (n - df + 0.5) / (df + 0.5)) * (K1 + 1.0)


def _nested_csr(per_query):
    """Per query a list of (kind, term ids) -> the host arrays of a mask entry: ptr [nq + 1], kind [n], inner ptr
    [n + 1], the term ids flat (all int32)."""
    ptr = np.zeros(len(per_query) + 1, dtype=np.int32)
    kinds: List[int] = []
    inner: List[int] = [0]
    flat: List[int] = []
    for q, items in enumerate(per_query):
        for kind, ids in items:
            kinds.append(kind)
            flat.extend(ids)
            inner.append(len(flat))
        ptr[q + 1] = len(kinds)
    return (ptr, np.asarray(kinds, dtype=np.int32), np.asarray(inner, dtype=np.int32), np.asarray(flat, dtype=np.int32))


def heaviest_slots(q_ptr, terms, weights, keep: int):
    """The CSR of `query_terms` with every query cut to its `keep` heaviest slots -- equal weights by the lower term id --,
    the kept slots back in ascending term-id order.  A batch within the limit comes back as it is."""
    if np.all(np.diff(q_ptr) <= keep):
        return q_ptr, terms, weights
    out_ptr = np.zeros_like(q_ptr)
    picks = []
    for q in range(len(q_ptr) - 1):
        a, b = int(q_ptr[q]), int(q_ptr[q + 1])
        idx = np.arange(a, b)
        if b - a > keep:
            order = np.lexsort((terms[a:b], -weights[a:b].astype(np.float64)))[:keep]   # weight descending, then term id
            idx = a + order[np.argsort(terms[a:b][order], kind="stable")]
        picks.append(idx)
        out_ptr[q + 1] = out_ptr[q] + idx.size
    take = np.concatenate(picks)
    return out_ptr, terms[take], weights[take]


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
