"""Repetition control for the native decoder: the parameters, and the rule crag_enc_adjust_logits (csrc/crag_penalty.hip)
implements, in numpy and fp32 with the operations in the kernel's order -- the tests' oracle, held bit for bit.

  PenaltyParams   repetition_penalty, presence_penalty, frequency_penalty, no_repeat_ngram, logit_bias, min_new_tokens,
                  with the range checks of the C entry
  bias_list       a row's bias list: logit_bias, and the stop ids at -inf while fewer than min_new_tokens ids are out
  exempt_ids      the ids whose bytes all lie in an alphabet (the citation alphabet of /answer)
  adjust_host     one row: the adjusted logits and the token picked on them

The rule.  H = history[:total] is everything the sequence holds, P = H[:prompt_len] its prompt, O = H[prompt_len:] its
output so far; seen(t): t occurs in H; c(t): how often t occurs in O.  Per id t, from l = logits[t]:
  1. only when t is not exempt:
     a. seen(t) and repetition_penalty != 1:  l = l / rp when l > 0, else l * rp  (one correctly rounded fp32 operation;
        a NaN takes the else arm and stays NaN)
     b. c(t) > 0:  l = (l - fp32(frequency * fp32(c))) - presence  (three roundings, no fused multiply-add)
     c. no_repeat_ngram = n > 0, |O| >= n - 1, and some j with j + n - 1 < |O| has O[j .. j+n-2] equal to the last n - 1
        ids of O and O[j+n-1] == t:  l = -inf
  2. t is in the row's bias list:  l = l + b
The token is the lowest id among the maxima of the adjusted row, NaNs left out, -1 when nothing is left:
crag_enc_lm_head's rule.  An id of the history outside 0..vocab - 1 is ignored (it still takes part in n-gram matches).

Three decisions.
  * Repetition looks at prompt and output, as HF transformers and vLLM do.
  * Presence, frequency and the n-gram ban look at the OUTPUT only: a grounded answer has to be free to quote its
    evidence, which sits in the prompt.
  * min_new_tokens is no rule of its own: while fewer ids than that have been produced, the stop ids join the bias list
    with -inf (bias_list).
exempt_ids(table, alphabet) names the ids whose bytes are non-empty and all in `alphabet`; /answer passes
CITATION_ALPHABET, so that citing [Q-12] a second time is never penalised or banned.  Bias still applies to exempt ids.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Mapping, Optional, Sequence, Tuple

import numpy as np

MIN_REPETITION, MAX_REPETITION = 0.1, 10.0      # CRAG_ADJUST_MIN_REPETITION / CRAG_ADJUST_MAX_REPETITION
MAX_ADDITIVE = 2.0                              # CRAG_ADJUST_MAX_ADDITIVE: |presence|, |frequency|
MIN_NGRAM, MAX_NGRAM = 2, 8                     # CRAG_ADJUST_MAX_NGRAM
MAX_BIAS = 256                                  # CRAG_ADJUST_MAX_BIAS: entries of a row's bias list
MAX_BIAS_VALUE = 100.0
CITATION_ALPHABET = b"[]-0123456789QA"


def _is_int(value) -> bool:
    return not isinstance(value, bool) and isinstance(value, (int, np.integer))


@dataclass(frozen=True)
class PenaltyParams:
    """Every field at its default changes nothing (`neutral`); a neutral value is treated exactly as None."""
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    no_repeat_ngram: int = 0
    logit_bias: Mapping[int, float] = field(default_factory=dict)
    min_new_tokens: int = 0

    def __post_init__(self) -> None:
        rp = float(self.repetition_penalty)
        if not MIN_REPETITION <= rp <= MAX_REPETITION:
            raise ValueError(f"repetition_penalty must be in {MIN_REPETITION}..{MAX_REPETITION} (got {self.repetition_penalty})")
        for name in ("presence_penalty", "frequency_penalty"):
            if not -MAX_ADDITIVE <= float(getattr(self, name)) <= MAX_ADDITIVE:
                raise ValueError(f"{name} must be in -{MAX_ADDITIVE}..{MAX_ADDITIVE} (got {getattr(self, name)})")
        n = self.no_repeat_ngram
        if not _is_int(n) or not (n == 0 or MIN_NGRAM <= n <= MAX_NGRAM):
            raise ValueError(f"no_repeat_ngram must be 0 or an integer in {MIN_NGRAM}..{MAX_NGRAM} (got {n!r})")
        if not _is_int(self.min_new_tokens) or self.min_new_tokens < 0:
            raise ValueError(f"min_new_tokens must be a non-negative integer (got {self.min_new_tokens!r})")
        if not isinstance(self.logit_bias, Mapping):
            raise ValueError("logit_bias must map token ids to values")
        if len(self.logit_bias) > MAX_BIAS:
            raise ValueError(f"logit_bias takes at most {MAX_BIAS} ids (got {len(self.logit_bias)})")
        bias: Dict[int, float] = {}
        for key, value in self.logit_bias.items():
            try:   # a JSON object's keys are strings
                tid = int(key)
            except (TypeError, ValueError):
                raise ValueError(f"logit_bias: {key!r} is not a token id") from None
            if isinstance(key, (bool, float)) or tid < 0 or tid > 0x7FFFFFFF or tid in bias:
                raise ValueError(f"logit_bias: {key!r} is not a token id of its own")
            try:
                b = float(value)
            except (TypeError, ValueError):
                raise ValueError(f"logit_bias[{key!r}] is not a number") from None
            if not (b == -math.inf or -MAX_BIAS_VALUE <= b <= MAX_BIAS_VALUE):   # a NaN fails both
                raise ValueError(f"logit_bias[{key!r}] must be finite in -{MAX_BIAS_VALUE}..{MAX_BIAS_VALUE} or -inf (got {value})")
            bias[tid] = b
        object.__setattr__(self, "logit_bias", dict(sorted(bias.items())))

    def __hash__(self) -> int:
        return hash((self.repetition_penalty, self.presence_penalty, self.frequency_penalty, self.no_repeat_ngram,
                     tuple(self.logit_bias.items()), self.min_new_tokens))

    @property
    def neutral(self) -> bool:
        return float(self.repetition_penalty) == 1.0 and float(self.presence_penalty) == 0.0 \
            and float(self.frequency_penalty) == 0.0 and int(self.no_repeat_ngram) == 0 and not self.logit_bias \
            and int(self.min_new_tokens) == 0

    def echo(self) -> dict:
        """The parameters as /answer reports them (-inf as the string "-inf": JSON has no such number)."""
        return {"repetition_penalty": float(self.repetition_penalty), "presence_penalty": float(self.presence_penalty),
                "frequency_penalty": float(self.frequency_penalty), "no_repeat_ngram": int(self.no_repeat_ngram),
                "logit_bias": {str(t): (b if b != -math.inf else "-inf") for t, b in self.logit_bias.items()},
                "min_new_tokens": int(self.min_new_tokens)}


def active(params: Optional[PenaltyParams]) -> Optional[PenaltyParams]:
    """None for None and for a neutral value: the decoder then runs the code path without penalties."""
    return None if params is None or params.neutral else params


def bias_list(params: PenaltyParams, produced: int = 0, stop_ids: Iterable[int] = (), vocab: Optional[int] = None
              ) -> List[Tuple[int, float]]:
    """The bias list of a row that has produced `produced` ids: logit_bias, and -- min_new_tokens -- the stop ids at
    -inf while produced < min_new_tokens; ascending ids, those at or beyond `vocab` left out.  ValueError: more than
    MAX_BIAS entries."""
    bias = dict(params.logit_bias)
    if int(produced) < int(params.min_new_tokens):
        for s in stop_ids:
            if int(s) >= 0:
                bias[int(s)] = -math.inf
    out = sorted((t, b) for t, b in bias.items() if vocab is None or t < int(vocab))
    if len(out) > MAX_BIAS:
        raise ValueError(f"a row's bias list takes at most {MAX_BIAS} ids (logit_bias and the stop ids under min_new_tokens)")
    return out


def exempt_ids(table, alphabet: bytes = CITATION_ALPHABET) -> np.ndarray:
    """The ids of a grammar.TokenTable whose bytes are non-empty and all in `alphabet`, ascending (int64)."""
    inside = np.zeros(256, dtype=bool)
    inside[np.frombuffer(bytes(alphabet), dtype=np.uint8)] = True
    offsets = np.asarray(table.offsets, dtype=np.int64)
    lens = np.diff(offsets)
    ok = inside[np.asarray(table.bytes, dtype=np.uint8)[:int(offsets[-1])]].astype(np.int64)
    reach = np.concatenate([[0], np.cumsum(ok)])
    return np.nonzero((lens > 0) & (reach[offsets[1:]] - reach[offsets[:-1]] == lens))[0]


def exempt_words(ids: Iterable[int], vocab: int) -> np.ndarray:
    """uint32 [ceil(vocab / 32)]: bit t % 32 of word t / 32 set for every id t -- the kernel's exempt_bits."""
    words = np.zeros((int(vocab) + 31) // 32, dtype=np.uint32)
    idx = np.asarray([t for t in ids if 0 <= int(t) < int(vocab)], dtype=np.int64)
    np.bitwise_or.at(words, idx >> 5, (np.uint32(1) << (idx & 31).astype(np.uint32)))
    return words


def banned_continuations(output: Sequence[int], n: int) -> List[int]:
    """Clause c: the ids that would complete an n-gram the output already holds."""
    out, n = [int(t) for t in output], int(n)
    if n <= 0 or len(out) < n - 1:
        return []
    tail = out[len(out) - (n - 1):]
    return sorted({out[j + n - 1] for j in range(len(out) - n + 1) if out[j:j + n - 1] == tail})


def adjust_host(logits_row, history: Sequence[int], prompt_len: int, params: PenaltyParams, exempt=None, bias=None,
                total: Optional[int] = None) -> Tuple[np.ndarray, int]:
    """(adjusted row fp32 [V], token) by the rule of the module docstring.  history: the sequence's ids, of which the
    first `total` (default all) count; exempt: bool [V], or ids; bias: the row's list of (id, value) or a mapping
    (default params.logit_bias)."""
    row = np.array(logits_row, dtype=np.float32)
    vocab = row.size
    hist = np.asarray(history, dtype=np.int64)[:len(history) if total is None else int(total)]
    prompt_len = int(prompt_len)
    if not 0 <= prompt_len <= hist.size:
        raise ValueError("prompt_len must lie inside the history")
    output = hist[prompt_len:]
    inside = lambda ids: ids[(ids >= 0) & (ids < vocab)]   # noqa: E731
    seen = np.zeros(vocab, dtype=bool)
    seen[inside(hist)] = True
    count = np.bincount(inside(output), minlength=vocab)
    if exempt is None:
        free = np.ones(vocab, dtype=bool)
    else:
        ex = np.asarray(exempt)
        free = ~ex if ex.dtype == bool else np.ones(vocab, dtype=bool)
        if ex.dtype != bool:
            free[inside(ex.astype(np.int64))] = False
    rp = np.float32(params.repetition_penalty)
    with np.errstate(all="ignore"):
        if float(params.repetition_penalty) != 1.0:                                                  # a
            at = seen & free
            row[at] = np.where(row[at] > 0, row[at] / rp, row[at] * rp).astype(np.float32)
        at = (count > 0) & free                                                                          # b
        step = (np.float32(params.frequency_penalty) * count[at].astype(np.float32)).astype(np.float32)
        row[at] = ((row[at] - step).astype(np.float32) - np.float32(params.presence_penalty)).astype(np.float32)
        for t in banned_continuations(output.tolist(), params.no_repeat_ngram):                          # c
            if 0 <= t < vocab and free[t]:
                row[t] = -np.inf
        pairs = params.logit_bias.items() if bias is None else (bias.items() if isinstance(bias, Mapping) else bias)
        for t, b in pairs:                                                                               # 2
            if 0 <= int(t) < vocab:
                row[int(t)] = np.float32(row[int(t)] + np.float32(b))
    idx = np.nonzero(~np.isnan(row))[0]
    token = int(idx[np.argmax(row[idx])]) if idx.size else -1
    return row, token
