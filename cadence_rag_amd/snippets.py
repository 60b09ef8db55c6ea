"""Query-aware snippets of /retrieve, host side: where the tokens of a text stand, how a snippet is cut
around a window the BM25 word lane chose, and that lane's window rule in numpy for callers without a GPU.

The reference cuts `_clip(text, 800)`, the head of the chunk, and asks for more ("Ensure artifact snippets are actually
relevant (not just 'first N chars of the doc')", APP_SPEC.md:269) without code for it: the rule is this tree's own.
include/crag_dense.h states it at crag_bm25_snippets_host; csrc/crag_bm25_snippet.hip runs it on the device."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from .bm25 import _RUN, MAX_TOKEN_BYTES

LEAD_TOKENS = 8     # tokens of context a cut keeps in front of the window's first token
ELLIPSIS = "…"


def clip(text: str, max_chars: int) -> str:
    """The head clip of the reference (retrieve.py:24-29)."""
    if max_chars <= 0:
        return ""
    if len(text) <= max_chars:
        return text
    return text[: max_chars - 1].rstrip() + ELLIPSIS


def token_spans(text: str) -> List[Tuple[int, int]]:
    """The (begin, end) character span of every token `bm25.tokenize` yields, in order: text[b:e].lower() is the token.
    Token position p of a row in a Bm25Index is spans[p] of the row's text."""
    out = []
    for m in _RUN.finditer(text or ""):
        tok = m.group().lower()
        if len(tok) <= MAX_TOKEN_BYTES // 4 or len(tok.encode("utf-8")) <= MAX_TOKEN_BYTES:
            out.append(m.span())
    return out


def cut_snippet(text: str, start: int, last: int, max_chars: int) -> str:
    """The snippet of `text` for the window whose first matched token is `start` and whose last is `last` (token
    positions; start < 0: the lane found no query word in the row).
      - the whole text when it fits in max_chars;
      - the head clip when start < 0 (or when the text has no token `start`: the lane indexed another text);
      - otherwise the text from the character where token max(0, start - LEAD_TOKENS) begins -- from character 0 when
        that is token 0 --, behind a leading "…" unless it begins at character 0, clipped like the head clip to max_chars
        in total.
    The cut begins there whether or not token `last` still falls inside it: the window's first words are shown, and as
    many of the following as the budget allows.  `last` is carried for callers that mark or measure the window."""
    if max_chars <= 0:
        return ""
    if len(text) <= max_chars or start < 0:
        return clip(text, max_chars)
    spans = token_spans(text)
    first = max(0, int(start) - LEAD_TOKENS)
    if int(start) >= len(spans) or first == 0:
        return clip(text, max_chars)
    return clip(ELLIPSIS + text[spans[first][0]:], max_chars)


def windows_host(post_ptr, post_pos, post_off, post_where, q_ptr, terms, weights, r_ptr, rows, window: int):
    """The rule of crag_bm25_snippets_host in numpy, fp32 sums in slot order: (start int32, last int32, score fp32,
    covered uint64), one entry per pair along r_ptr.  The arrays are Bm25Index.host_csr() / host_positions() and the
    CSR of Bm25Index.query_terms; rows are row positions."""
    if not 1 <= int(window) <= 65535:
        raise ValueError("window must be in [1, 65535]")
    post_ptr, post_pos = np.asarray(post_ptr), np.asarray(post_pos)
    post_off, post_where = np.asarray(post_off), np.asarray(post_where)
    weights = np.asarray(weights, dtype=np.float32)
    npairs = int(r_ptr[-1])
    start = np.full(npairs, -1, dtype=np.int32)
    last = np.zeros(npairs, dtype=np.int32)
    score = np.zeros(npairs, dtype=np.float32)
    covered = np.zeros(npairs, dtype=np.uint64)
    for q in range(len(r_ptr) - 1):
        t0, t1 = int(q_ptr[q]), int(q_ptr[q + 1])
        if t1 - t0 > 64:
            raise ValueError("a query has at most 64 term slots")
        for pair in range(int(r_ptr[q]), int(r_ptr[q + 1])):
            r = int(rows[pair])
            slices = []
            for t in terms[t0:t1]:
                a, b = int(post_ptr[t]), int(post_ptr[t + 1])
                pi = a + int(np.searchsorted(post_pos[a:b], r))
                held = pi < b and post_pos[pi] == r
                slices.append(post_where[post_off[pi]:post_off[pi + 1]].astype(np.int64) if held else np.empty(0, np.int64))
            occ = np.unique(np.concatenate(slices)) if slices else np.empty(0, np.int64)
            if occ.size == 0:
                continue
            sums = np.zeros(occ.size, dtype=np.float32)
            for j, sl in enumerate(slices):
                if sl.size:
                    at = np.searchsorted(sl, occ)
                    hit = (at < sl.size) & (sl[np.minimum(at, sl.size - 1)] < occ + int(window))
                    sums = np.where(hit, sums + weights[t0 + j], sums)     # (fp32 + fp32: one rounded addition)
            best = int(np.argmax(sums))                                     # (the first of the largest: the lowest start)
            s = int(occ[best])
            bits, hi = 0, -1
            for j, sl in enumerate(slices):
                inside = sl[(sl >= s) & (sl < s + int(window))]
                if inside.size:
                    bits |= 1 << j
                    hi = max(hi, int(inside[-1]))
            start[pair], last[pair], score[pair], covered[pair] = s, hi, sums[best], np.uint64(bits)
    return start, last, score, covered

