"""Seeded sampling for the native decoder: the parameters, and the rule crag_enc_sample (csrc/crag_sample.hip) implements,
in numpy and fp64 -- the tests' oracle.

  SamplingParams        temperature, top_k, top_p, min_p, seed, with the range checks of the C entry
  min_p_cut             fp32(T * ln min_p): the form the kernel takes the min-p cut in
  philox4x32_10         the counter-based generator (Salmon et al., Random123), vectorised over counters
  philox_uniform_host   u = ((x0 >> 8) + 0.5) * 2^-24 for counter (token id, step, stream, 0) and key (seed lo, seed hi)
  sample_host           one row: candidates, the cuts as thresholds on the logit, the Gumbel-maximum draw

The rule.  Candidates are the allowed ids whose logit is neither NaN nor -inf; m is their maximum.  No candidate: token
-1.  m == +inf or T == 0: the lowest id holding m.  Otherwise three thresholds on the logit, so ties stay together:
t_k the top_k-th largest candidate logit; t_m from (l - m) >= min_p_cut in fp32; and, inside S = {l >= max(t_k, t_m)} with
weights w = exp((l - m) / T), t_p the largest logit value whose weights from the top reach top_p of the weights of S.
The kept ids are those at or above max(t_k, t_m, t_p); `cut` is the lowest kept logit.  The token is the kept id with the
largest key (l - m) / T - ln(-ln u), the lowest id among equals: the Gumbel maximum draws from the softmax of the kept
logits, and does not depend on any order.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence

import numpy as np

MIN_TEMPERATURE = 0.01      # CRAG_SAMPLE_MIN_TEMPERATURE / CRAG_SAMPLE_MAX_TEMPERATURE
MAX_TEMPERATURE = 100.0


@dataclass(frozen=True)
class SamplingParams:
    """temperature 0 is greedy decoding (the other fields are then ignored); top_k 0, top_p 1 and min_p 0 cut nothing."""
    temperature: float
    top_k: int = 0
    top_p: float = 1.0
    min_p: float = 0.0
    seed: int = 0

    def __post_init__(self) -> None:
        t = float(self.temperature)
        if not (t == 0.0 or MIN_TEMPERATURE <= t <= MAX_TEMPERATURE):
            raise ValueError(f"temperature must be 0 or in {MIN_TEMPERATURE}..{MAX_TEMPERATURE} (got {self.temperature})")
        if int(self.top_k) != self.top_k or int(self.top_k) < 0:
            raise ValueError(f"top_k must be a non-negative integer (got {self.top_k})")
        if not 0.0 < float(self.top_p) <= 1.0:
            raise ValueError(f"top_p must be in (0, 1] (got {self.top_p})")
        if not 0.0 <= float(self.min_p) <= 1.0:
            raise ValueError(f"min_p must be in 0..1 (got {self.min_p})")
        if int(self.seed) != self.seed or not 0 <= int(self.seed) < 2 ** 64:
            raise ValueError(f"seed must be an integer in 0..2^64 - 1 (got {self.seed})")

    @property
    def greedy(self) -> bool:
        return float(self.temperature) == 0.0

    def echo(self) -> dict:
        """The parameters as /answer reports them."""
        return {"temperature": float(self.temperature), "top_k": int(self.top_k), "top_p": float(self.top_p),
                "min_p": float(self.min_p), "seed": int(self.seed)}


def min_p_cut(temperature: float, min_p: float) -> np.float32:
    """fp32(T * ln min_p), -inf for min_p == 0: the kernel keeps a logit when (l - m) >= this, in fp32."""
    if float(min_p) <= 0.0:
        return np.float32(-np.inf)
    return np.float32(float(np.float32(temperature)) * math.log(float(min_p)))


# ---- Philox4x32-10 ----------------------------------------------------------------------------------------------------
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(counter: Sequence, key: Sequence[int]) -> np.ndarray:
    """counter: four words (ints or equal-length arrays), key: two words -> uint32 [n, 4]."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & _LOW for x in counter]
    n = max(x.size for x in c)
    c0, c1, c2, c3 = (np.broadcast_to(x, (n,)).copy() for x in c)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> _32, p0 & _LOW, p1 >> _32, p1 & _LOW
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def philox_uniform_host(seed: int, step: int, stream: int, ids) -> np.ndarray:
    """float64 [len(ids)]: u = ((x0 >> 8) + 0.5) * 2^-24, strictly inside (0, 1)."""
    ids = np.asarray(ids, dtype=np.uint64)
    x0 = philox4x32_10((ids, int(step), int(stream), 0), (int(seed) & 0xFFFFFFFF, int(seed) >> 32))[:, 0]
    return ((x0 >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


# ---- the rule ---------------------------------------------------------------------------------------------------------
class HostDraw(NamedTuple):
    token: int          # -1: no candidate
    gap: float          # the largest key minus the second largest among the kept ids (inf: one kept id, or no draw)
    kept_lo: int        # the kept count under top_p * (1 - delta) ...
    kept_hi: int        # ... and under top_p * (1 + delta): a kernel's count must lie between them
    kept: int           # the kept count under top_p itself
    cut: float          # the lowest kept logit (NaN: no candidate)
    stable: bool        # the token is the same under top_p * (1 - delta) and top_p * (1 + delta)


def _kept_mask(values: np.ndarray, in_s: np.ndarray, m: float, temperature: float, top_p: float) -> np.ndarray:
    """The ids of S at or above t_p."""
    if top_p >= 1.0:
        return in_s
    idx = np.nonzero(in_s)[0]
    levels, inverse = np.unique(values[idx], return_inverse=True)            # ascending
    w = np.exp((values[idx] - m) / temperature)
    per_level = np.bincount(inverse, weights=w, minlength=levels.size)[::-1]   # descending logit
    reach = np.cumsum(per_level)
    at = int(np.searchsorted(reach, top_p * reach[-1], side="left"))          # the first level whose sum reaches it
    t_p = levels[::-1][min(at, levels.size - 1)]
    return in_s & (values >= t_p)


def sample_host(logits, params: SamplingParams, step: int, stream: int, allowed: Optional[np.ndarray] = None,
                delta: float = 1e-4) -> HostDraw:
    """The rule of the module docstring on one row of fp32 logits, in fp64.  allowed: bool [V] (None: every id)."""
    l32 = np.asarray(logits, dtype=np.float32)
    values = l32.astype(np.float64)
    temperature = float(np.float32(params.temperature))      # what the kernel receives
    top_p = float(np.float32(params.top_p))
    cand = ~np.isnan(values) & (values != -np.inf)
    if allowed is not None:
        cand &= np.asarray(allowed, dtype=bool)
    if int(params.top_k) > l32.size:
        raise ValueError(f"top_k must be in 0..{l32.size}")
    if not cand.any():
        return HostDraw(-1, math.inf, 0, 0, 0, math.nan, True)
    m = float(values[cand].max())
    if temperature == 0.0 or m == math.inf:
        top = cand & (values == m)
        n = int(top.sum())
        return HostDraw(int(np.nonzero(top)[0][0]), math.inf, n, n, n, m, True)
    with np.errstate(over="ignore", invalid="ignore"):
        in_s = cand & ((l32 - np.float32(m)) >= min_p_cut(temperature, params.min_p))   # fp32 on both sides
    k = int(params.top_k)
    if 0 < k < int(in_s.sum()):
        t_k = np.sort(values[in_s])[-k]
        in_s &= values >= t_k
    ids = np.nonzero(in_s)[0]
    key = np.full(values.shape, -np.inf)
    with np.errstate(over="ignore"):
        key[ids] = (values[ids] - m) / temperature - np.log(-np.log(philox_uniform_host(params.seed, step, stream, ids)))

    def draw(p: float):
        kept = _kept_mask(values, in_s, m, temperature, p)
        kk = np.where(kept, key, -np.inf)
        token = int(np.argmax(kk))                     # the first among equals: the lowest id
        rest = np.delete(kk, token)
        gap = float(kk[token] - rest.max()) if rest.size and rest.max() > -np.inf else math.inf
        return token, gap, int(kept.sum()), float(values[kept].min())

    token, gap, kept, cut = draw(top_p)
    if top_p >= 1.0:
        return HostDraw(token, gap, kept, kept, kept, cut, True)
    lo = draw(top_p * (1.0 - delta))
    hi = draw(min(top_p * (1.0 + delta), 1.0))
    return HostDraw(token, gap, lo[2], hi[2], kept, cut, lo[0] == token == hi[0])
