"""Prompt-lookup drafts for speculative decoding (host only, pure).

An answer quotes what already stands in its prompt -- snippets, evidence ids.  propose_drafts guesses the next tokens
of a sequence from the sequence itself: the tokens that followed the latest earlier occurrence of its current n-gram.
Qwen3Generator.generate(speculate=k) verifies up to k such drafts in one forward (step_rows) and keeps the prefix the
model itself would have produced (accepted_prefix), so the output never depends on what was proposed."""
from __future__ import annotations

from typing import List, Sequence

MAX_SPECULATE = 7   # drafts per forward: with the pending token they fill the 8 rows of one decode step


def propose_drafts(ids: Sequence[int], max_draft: int, max_ngram: int = 3, min_ngram: int = 1) -> List[int]:
    """Up to max_draft ids that followed the latest earlier occurrence of the longest suffix n-gram of `ids` (n from
    max_ngram down to min_ngram) that occurs earlier in `ids` at all; never past the end of `ids`.  [] when nothing
    matches, when max_draft <= 0, or when an id is negative (an unknown token)."""
    ids = [int(x) for x in ids]
    max_draft, total = int(max_draft), len(ids)
    if max_draft <= 0 or any(x < 0 for x in ids):
        return []
    for n in range(min(int(max_ngram), total - 1), max(int(min_ngram), 1) - 1, -1):
        suffix = ids[total - n:]
        for start in range(total - n - 1, -1, -1):     # the latest earlier occurrence first
            if ids[start:start + n] == suffix:
                return ids[start + n:start + n + max_draft]
    return []


def accepted_prefix(drafts: Sequence[int], picks: Sequence[int]) -> int:
    """How many leading drafts are right: draft i is right when the drafts before it are and it equals picks[i], the
    token picked at the row before it (row 0 carries the pending token, row i > 0 draft i - 1)."""
    n = 0
    while n < len(drafts) and n < len(picks) and int(drafts[n]) == int(picks[n]):
        n += 1
    return n
