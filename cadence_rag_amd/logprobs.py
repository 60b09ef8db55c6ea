"""Token log-probabilities for the native decoder: the rule crag_enc_logprobs (csrc/crag_logprobs.hip) implements, in
numpy and fp64 on the fp32 logits -- the tests' oracle, as sampling.sample_host is crag_enc_sample's -- the error bar a
kernel's fp32 outputs are held to, and the small helpers /answer summarises a reply's records with.

  logprobs_host     one row: lse_all, lse_allowed, the token's logprob and rank, the n_top best (id, logprob)
  error_bar         DESIGN 6d's bound on |kernel - rule| for one output
  TokenLogprob      the record the generator keeps per produced token
  mean_logprob      the length-normalised likelihood of a reply

The rule.  A candidate is an id whose logit is not NaN (-inf is one); an allowed candidate has its flag set (allowed is
None: every candidate).  lse over a set = m + ln sum exp(l - m) with m the set's own maximum; -inf for an empty set and
for a set of -inf alone, +inf when m is +inf.  logprob = l_token - lse_all by IEEE rules (finite - inf = -inf, inf - inf =
NaN), NaN for a token outside the row or with a NaN logit: the model's own distribution at temperature 1, whatever picked
the token.  rank = 1 + the candidates strictly above l_token (-0 == +0), 0 for such a token.  The top entries are the
first n_top candidates of ALL ids by (logit descending, id ascending), each with l - lse_all; fewer candidates than n_top
are padded with id -1 and NaN.  allowed_logmass = lse_allowed - lse_all <= 0: the log of the probability the allowed
ids hold.
"""
from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional, Sequence

import numpy as np

MAX_TOP = 16   # CRAG_LOGPROBS_MAX_TOP


class HostLogprobs(NamedTuple):
    logprob: float              # NaN: the token is outside the row, or its logit is NaN
    rank: int                   # 0 with such a token
    lse_all: float
    lse_allowed: float          # == lse_all without a mask
    allowed_logmass: float      # lse_allowed - lse_all (NaN when both are infinite)
    top_id: np.ndarray          # int32 [n_top], -1 behind the last candidate
    top_logprob: np.ndarray     # float64 [n_top], NaN behind the last candidate
    m_all: float                # the maximum over the candidates (NaN: none)
    ln_z_all: float             # lse_all - m_all where both are finite, else 0: what error_bar takes
    m_allowed: float
    ln_z_allowed: float


def _lse(values: np.ndarray) -> tuple:
    """(lse, m, ln Z) of a set of fp64 values without NaN."""
    if values.size == 0:
        return -math.inf, math.nan, 0.0
    m = float(values.max())
    if math.isinf(m):
        return m, m, 0.0
    ln_z = math.log(float(np.exp(values - m).sum()))
    return m + ln_z, m, ln_z


def logprobs_host(logits_row, token: int, allowed: Optional[np.ndarray] = None, n_top: int = 0) -> HostLogprobs:
    """The rule of the module docstring on one row of fp32 logits, in fp64.  allowed: bool [V] (None: every id)."""
    l32 = np.asarray(logits_row, dtype=np.float32).reshape(-1)
    values = l32.astype(np.float64)
    vocab = values.size
    n_top = int(n_top)
    if not 0 <= n_top <= MAX_TOP or n_top > vocab:
        raise ValueError(f"n_top must be in 0..{MAX_TOP} and at most the row's length")
    cand = ~np.isnan(values)
    lse_all, m_all, z_all = _lse(values[cand])
    if allowed is None:
        lse_alw, m_alw, z_alw = lse_all, m_all, z_all
    else:
        lse_alw, m_alw, z_alw = _lse(values[cand & np.asarray(allowed, dtype=bool).reshape(-1)])
    token = int(token)
    with np.errstate(invalid="ignore"):
        if 0 <= token < vocab and cand[token]:
            lt = float(values[token])
            logprob = float(np.float64(lt) - np.float64(lse_all))
            rank = 1 + int((values[cand] > lt).sum())
        else:
            logprob, rank = math.nan, 0
        mass = float(np.float64(lse_alw) - np.float64(lse_all))
        ids = np.nonzero(cand)[0]
        order = ids[np.argsort(-values[ids], kind="stable")][:n_top]   # equal logits keep the ascending ids
        top_id = np.full(n_top, -1, dtype=np.int32)
        top_lp = np.full(n_top, np.nan, dtype=np.float64)
        top_id[:order.size] = order
        top_lp[:order.size] = values[order] - np.float64(lse_all)
    return HostLogprobs(logprob, rank, lse_all, lse_alw, mass, top_id, top_lp, m_all, z_all, m_alw, z_alw)


def error_bar(value: float, lse: float, ln_z: float) -> float:
    """The bound on |kernel - rule| for one finite fp32 output `value` (a logprob, a top logprob, or the lse itself)
    that was computed from the log-sum-exp `lse` = m + ln Z: 2^-24 * (24 + 4 |ln Z| + |lse| + |value|), derived in DESIGN
    6d for vocabularies up to 2^18.  Infinite and NaN outputs are compared exactly, not with a bar."""
    return 2.0 ** -24 * (24.0 + 4.0 * abs(ln_z) + abs(lse) + abs(value))


# ---- the generator's records --------------------------------------------------------------------------------------------
class TokenLogprob(NamedTuple):
    token: int
    logprob: float
    rank: int
    allowed_logmass: Optional[float]    # under a grammar: ln of the probability the automaton left allowed; else None
    top: List[tuple]                    # the n most likely (id, logprob) of the whole row


def mean_logprob(records: Sequence[TokenLogprob]) -> Optional[float]:
    """The mean token log-probability of a reply -- its length-normalised likelihood; None for no token."""
    if not records:
        return None
    return float(sum(float(r.logprob) for r in records) / len(records))


def summarise(records: Sequence[TokenLogprob]) -> Dict[str, object]:
    """What /answer reports about the returned answer: {"tokens", "mean_logprob", "min_logprob"}, and under a grammar
    {"mean_allowed_logmass", "min_allowed_logmass"} as well."""
    lps = [float(r.logprob) for r in records]
    out: Dict[str, object] = {"tokens": len(lps), "mean_logprob": mean_logprob(records),
                              "min_logprob": min(lps) if lps else None}
    masses = [float(r.allowed_logmass) for r in records if r.allowed_logmass is not None]
    if masses:
        out["mean_allowed_logmass"] = float(sum(masses) / len(masses))
        out["min_allowed_logmass"] = min(masses)
    return out
