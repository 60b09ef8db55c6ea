"""CPU oracle of the BM25 lane: numpy, fp64 throughout, written independently of cadence_rag_amd/bm25.py (only the
tokeniser is shared -- it is the specification's one function for rows and queries).

    score = sum_t qtf(t) * idf(t) * (k1 + 1) * tf / (tf + k1 * (1 - b + b * dl / avgdl))
    idf(t) = ln(1 + (N - df + 0.5) / (df + 0.5)),  k1 = 1.2,  b = 0.75

Per query: dense tf matrix [N, T] over the query's distinct known terms -> scores -> (-score, id) sort -> mask -> first k.
"""
from collections import Counter

import numpy as np

from cadence_rag_amd.bm25 import tokenize

K1, B = 1.2, 0.75
EPS = 2.0 ** -24


class Bm25Oracle:
    def __init__(self, texts, ids):
        self.ids = np.asarray(ids, dtype=np.int64)
        self.n = len(texts)
        rows = [Counter(tokenize(t)) for t in texts]
        self.dl = np.array([sum(c.values()) for c in rows], dtype=np.float64)
        self.avgdl = float(self.dl.sum() / self.n) if self.n else 0.0
        post = {}
        for i, c in enumerate(rows):
            for tok, tf in c.items():
                post.setdefault(tok, []).append((i, tf))
        self.post = {tok: (np.array([p for p, _ in v]), np.array([min(tf, 65535) for _, tf in v], dtype=np.float64))
                     for tok, v in post.items()}

    def scores(self, query):
        """(scores fp64 [N], T = distinct known terms of the query); a row without any query term scores 0."""
        qtf = Counter(tok for tok in tokenize(query) if tok in self.post)
        terms = sorted(qtf)
        tfm = np.zeros((self.n, len(terms)), dtype=np.float64)
        w = np.zeros(len(terms), dtype=np.float64)
        for j, tok in enumerate(terms):
            pos, tf = self.post[tok]
            tfm[pos, j] = tf
            df = float(len(pos))
            w[j] = qtf[tok] * np.log(1.0 + (self.n - df + 0.5) / (df + 0.5)) * (K1 + 1.0)
        if not terms:
            return np.zeros(self.n), 0
        norm = K1 * (1.0 - B + B * self.dl / self.avgdl)
        return (w[None, :] * tfm / (tfm + norm[:, None])).sum(axis=1), len(terms)

    def topk(self, query, k, eligible=None):
        """ids [k] (-1 pad), scores [k] (NaN pad), count: matches only, (-score, id) order, mask, first k."""
        s, _ = self.scores(query)
        order = np.lexsort((self.ids, -s))
        keep = s[order] > 0
        if eligible is not None:
            keep &= np.asarray(eligible, dtype=bool)[order]
        order = order[keep][:k]
        ids = np.full(k, -1, dtype=np.int64)
        sc = np.full(k, np.nan)
        ids[:len(order)] = self.ids[order]
        sc[:len(order)] = s[order]
        return ids, sc, len(order)


def tolerance(n_terms):
    """Relative: every summand is positive (no cancellation); a term's contribution carries at most 9 fp32 roundings
    (avgdl, dl/avgdl, *b, +(1-b), *k1, +tf, the division, the weight, the product) and adding T terms T - 1 more:
    |dscore| <= (T + 9) * 2^-24 * score.  The tests allow twice that."""
    return 2.0 * (n_terms + 9) * EPS


def assert_matches(oracle, query, k, got_ids, got_scores, got_count, eligible=None):
    """One query's result against the oracle.  Scores within tolerance(T) * score of the returned row's own oracle
    score; ids equal to the oracle's except that position j may hold any row whose oracle score is within that same
    relative window of the oracle's j-th score (a permutation inside a run of near ties; a run that straddles k swaps
    members in and out).  Rows with exactly equal oracle scores and equal returned bits must ascend by id."""
    s, t = oracle.scores(query)
    want_ids, want_sc, want_n = oracle.topk(query, k, eligible)
    tol = tolerance(t)
    got_ids, got_scores = np.asarray(got_ids), np.asarray(got_scores)
    assert int(got_count) == want_n, (query, int(got_count), want_n)
    assert np.all(got_ids[want_n:] == -1) and np.all(np.isnan(got_scores[want_n:]))
    if want_n == 0:
        return 0.0
    pos_of = {int(v): i for i, v in enumerate(oracle.ids)}
    assert len(set(got_ids[:want_n].tolist())) == want_n, "a row was returned twice"
    worst = 0.0
    for j in range(want_n):
        p = pos_of[int(got_ids[j])]
        assert s[p] > 0 and (eligible is None or eligible[p]), f"{query!r}: row {got_ids[j]} must not be returned"
        err = abs(float(got_scores[j]) - s[p]) / s[p]
        worst = max(worst, err / (tol / 2.0))
        assert err <= tol, f"{query!r}: score of id {got_ids[j]} off by {err:.3e} relative (allowed {tol:.3e})"
        if got_ids[j] != want_ids[j]:
            assert abs(s[p] - want_sc[j]) <= tol * want_sc[j], \
                f"{query!r}: position {j} holds id {got_ids[j]}, the oracle {want_ids[j]}, and they are no near tie"
        if j and got_scores[j - 1] == got_scores[j] and s[pos_of[int(got_ids[j - 1])]] == s[p]:
            assert got_ids[j - 1] < got_ids[j], f"{query!r}: exact tie out of id order at position {j}"
        if j:
            assert got_scores[j - 1] >= got_scores[j], f"{query!r}: scores ascend at position {j}"
    return worst   # worst error as a fraction of the single bound (T + 9) * 2^-24
