"""BM25 lane, the paths no other test runs, bit for bit against tests/bm25_replay.py (the fp32 restatement of the formula
in include/crag_dense.h): the merge kernel's second and third round with its carried best, the score kernel's rounds of
256 terms with a late first hit, the selection inside a range at its edges, the extreme values of tf, dl and the
weights, and every row's bits over two ranges (mask windows of k rows).  Corpora are synthetic numpy CSR arrays
(Bm25Index.from_arrays, or raw arrays through the C ABI), queried as term ids with chosen fp32 weights.

Every comparison is exact equality of ids, score bits, counts and padding; the planted expectations (which rows must
win, which must tie) come on top.  Every weight lies in 2^-40 ... 2^40 and no product w * tf / (tf + x) underflows:
what an underflowing product does is not pinned here.

A merge round takes (5 * 1024 - 128) // k range lists: 39 at k = 128, 49 at k = 100, 99 at k = 50; each merge case prints
the number of rounds it took, ceil(ranges / that)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from bm25_replay import NAN_BITS, assert_equals_replay, replay, replay_index
from cadence_rag_amd import _native
from cadence_rag_amd.bm25 import RANGE_ROWS as R
from cadence_rag_amd.bm25 import Bm25Index
from cadence_rag_amd.dense_index import DenseIndex

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MERGE_KEYS = 5 * 1024 - 128
WEIGHTS = np.random.default_rng(4242).uniform(0.5, 8.0, size=1024).astype(np.float32)    # by term id


def merge_rounds(n_rows, k):
    return math.ceil(math.ceil(n_rows / R) / (MERGE_KEYS // k))


class Corpus:
    """Postings collected term by term (term ids in order of creation), turned into the row CSR of from_arrays."""

    def __init__(self, n):
        self.n, self.pos, self.tf = n, [], []

    def term(self, pos, tf):
        pos = np.asarray(pos, dtype=np.int64).reshape(-1)
        tf = np.broadcast_to(np.asarray(tf, dtype=np.int64), pos.shape).copy()
        assert np.all(np.diff(pos) > 0) and (pos.size == 0 or (pos[0] >= 0 and pos[-1] < self.n)) and np.all(tf >= 1)
        self.pos.append(pos)
        self.tf.append(tf)
        return len(self.pos) - 1

    def row_sums(self):
        return np.bincount(np.concatenate(self.pos), weights=np.concatenate(self.tf), minlength=self.n).astype(np.int64)

    def index(self, ids):
        term = np.repeat(np.arange(len(self.pos)), [p.size for p in self.pos])
        pos, tf = np.concatenate(self.pos), np.concatenate(self.tf)
        order = np.lexsort((term, pos))
        row_ptr = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(np.bincount(pos, minlength=self.n), out=row_ptr[1:])
        return Bm25Index.from_arrays(row_ptr, term[order], tf[order], len(self.pos), ids, DEV)


def q(*terms):
    """A query of these term ids with the table's weights."""
    t = np.sort(np.asarray(terms, dtype=np.int32).reshape(-1))
    return t, WEIGHTS[t % WEIGHTS.size]


def run(index, queries, k, eligible=None, packed=None, what=""):
    """queries: (term ids ascending, fp32 weights) each.  Searches, compares exactly with the replay and returns host
    arrays (ids, score bits, counts).  eligible: None, bool [N] or bool [nq, N]; packed: the mask bytes to send instead
    of pack_mask(eligible)."""
    q_ptr = np.zeros(len(queries) + 1, dtype=np.int32)
    q_ptr[1:] = np.cumsum([len(t) for t, _ in queries])
    terms = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int32) for t, _ in queries]))
    w = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float32) for _, x in queries]))
    assert np.all(w >= 2.0 ** -40) and np.all(w <= 2.0 ** 40)
    mask, stride = None, 0
    if eligible is not None:
        packed = DenseIndex.pack_mask(eligible) if packed is None else packed
        mask = torch.from_numpy(packed).to(DEV)
        stride = packed.shape[-1] if packed.ndim == 2 else 0
    ids, sc, ct = [x.cpu().numpy() for x in index.search_terms(q_ptr, terms, w, k, row_mask=mask, mask_stride=stride)]
    assert ids.shape == (len(queries), k) and sc.shape == (len(queries), k) and ct.shape == (len(queries),)
    assert_equals_replay(replay_index(index, q_ptr, terms, w, k, eligible), ids, sc, ct, what or f"k={k}")
    bits = sc.view(np.uint32)
    for i in range(len(queries)):
        assert np.all(ids[i, ct[i]:] == -1) and np.all(bits[i, ct[i]:] == NAN_BITS)
        assert np.all(ids[i, :ct[i]] >= 0) and len(set(ids[i, :ct[i]].tolist())) == ct[i]
    return ids, bits, ct


def window(rng, rg, lo, m, width=1000):
    """m ascending positions inside local [lo, lo + width) of range rg."""
    return rg * R + lo + np.sort(rng.choice(width, size=m, replace=False))


def best_level_rows(index, pos, tf):
    """Rows of a one-term query's best (tf, dl) pair, ascending -- computed in fp64 from the distinct pairs."""
    dl = index.doc_len[pos].astype(np.int64)
    pair = tf.astype(np.int64) << 32 | dl
    levels = np.unique(pair)
    ltf, ldl = (levels >> 32).astype(np.float64), (levels & 0xFFFFFFFF).astype(np.float64)
    score = ltf / (ltf + 1.2 * (0.25 + 0.75 * ldl / float(index.avgdl)))
    top = np.argsort(score)[::-1]
    assert score[top[0]] > score[top[1]] * (1 + 1e-5), "the best level must be clear of fp32 rounding"
    return pos[pair == levels[top[0]]], levels.size


# ---- the merge kernel's rounds -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def merge_corpus(gpu):
    """80 ranges (79 * R + 5 rows).  k = 128: merge rounds of 39 + 39 + 2 lists; k = 100: 49 + 31; k = 50: one round."""
    n = 79 * R + 5
    rng = np.random.default_rng(77)
    c = Corpus(n)
    last = n - 1
    t = {}
    # (a) one posting at the first position of range 0 and at the last of ranges 38, 39, 77, 78, 79
    spots_a = np.array([0, 39 * R - 1, 40 * R - 1, 78 * R - 1, 79 * R - 1, last])
    t["a"] = c.term(spots_a, 2)
    # (b) k losers in range 0, more than k winners at the far end (range 78 and the first rows of range 79)
    lose_b = window(rng, 0, 1000, 128)
    win_b = np.concatenate([window(rng, 78, 1000, 130), 79 * R + np.arange(3)])
    t["b"] = c.term(np.concatenate([lose_b, win_b]), np.concatenate([np.ones(128, int), 5 + np.arange(133) % 5]))
    # (c) the reverse: winners in range 0, losers in a range of round two and one of round three
    win_c = window(rng, 0, 2000, 130)
    lose_c = np.concatenate([window(rng, 45, 2000, 130), window(rng, 78, 2000, 130)])
    t["c"] = c.term(np.concatenate([win_c, lose_c]), np.concatenate([5 + np.arange(130) % 5, np.ones(260, int)]))
    # (d) matches only behind the first round of k = 128 (39 lists) and of k = 100 (49 lists)
    spots_d = np.concatenate([window(rng, 50, 3000, 70), window(rng, 78, 3000, 70)])
    t["d"] = c.term(spots_d, 1 + np.arange(140) % 4)
    # (e) matches in rounds one and three only
    spots_e = np.concatenate([window(rng, 3, 4000, 100), window(rng, 20, 4000, 60), window(rng, 78, 4000, 90),
                              [79 * R + 3]])
    t["e"] = c.term(spots_e, 1 + np.arange(spots_e.size) % 6)
    planted = np.zeros(n, dtype=bool)
    for p in c.pos:
        assert not planted[p].any(), "planted rows must not overlap"
        planted[p] = True
    # (f) a term in every row: tf 1, 2, 3 by position (1 in the planted rows, so that a group's rows share one dl)
    ftf = 1 + np.arange(n) % 3
    ftf[planted] = 1
    t["f"] = c.term(np.arange(n), ftf)
    # background: 200 terms over the unplanted rows
    t["bg"] = []
    for _ in range(200):
        p = np.unique(rng.integers(0, n, size=int(rng.integers(20, 6000))))
        p = p[~planted[p]]
        t["bg"].append(c.term(p, rng.integers(1, 5, size=p.size)))
    index = c.index(np.arange(n, dtype=np.int64) * 5 + 11)
    info = dict(t, n=n, spots_a=spots_a, win_b=win_b, lose_b=lose_b, win_c=win_c, spots_d=spots_d, spots_e=spots_e,
                ftf=ftf, rng=rng)
    yield index, info
    index.close()


def planted_queries(info):
    bg = info["bg"]
    return [q(info["a"]), q(info["b"]), q(info["c"]), q(info["d"]), q(info["e"]), q(info["f"]),
            q(info["a"], info["b"], info["c"], info["d"], info["e"]), q(info["b"], info["f"]), q(*bg[:7]),
            q(info["c"], info["e"], *bg[50:90]), q(info["d"], bg[3]), q(*bg)]


@pytest.mark.parametrize("k", [128, 100, 50])
def test_merge_rounds_with_planted_terms(merge_corpus, k):
    index, info = merge_corpus
    n = info["n"]
    want_rounds = {128: 3, 100: 2, 50: 1}[k]
    assert merge_rounds(n, k) == want_rounds
    print(f"merge: {n} rows = {math.ceil(n / R)} ranges, k={k}: {MERGE_KEYS // k} lists a round, "
          f"{merge_rounds(n, k)} round(s)")
    ids, bits, ct = run(index, planted_queries(info), k)
    row = (ids - 11) // 5
    # (a) identical (tf, dl) at the first and last positions of the rounds' first and last ranges
    assert ct[0] == 6 and np.array_equal(row[0, :6], info["spots_a"]) and len(set(bits[0, :6].tolist())) == 1
    # (b) the carried best of round one is displaced wholly; (c) it passes through the later rounds unchanged
    assert ct[1] == k and set(row[1].tolist()) <= set(info["win_b"].tolist())
    assert ct[2] == k and set(row[2].tolist()) <= set(info["win_c"].tolist())
    # (d) nothing in the first round; (e) nothing in the middle round
    assert ct[3] == min(k, 140) and set(row[3, :ct[3]].tolist()) <= set(info["spots_d"].tolist())
    assert ct[4] == min(k, 251) and set(row[4, :ct[4]].tolist()) <= set(info["spots_e"].tolist())
    # (f) every list full of equal bits: the lowest ids of the best level
    level, n_levels = best_level_rows(index, np.arange(n), info["ftf"])
    assert level.size > 10 * R and n_levels < 200
    assert ct[5] == k and np.array_equal(row[5], level[:k]) and len(set(bits[5].tolist())) == 1
    # ... and with those ids masked out, the next ones; (b) without its winners falls back to round one's rows
    eligible = np.ones(n, dtype=bool)
    eligible[level[:k]] = False
    eligible[info["win_b"]] = False
    ids, bits, ct = run(index, [q(info["f"]), q(info["b"]), q(*info["bg"][:7]), q(info["a"])], k, eligible)
    row = (ids - 11) // 5
    assert ct[0] == k and np.array_equal(row[0], level[k:2 * k]) and len(set(bits[0].tolist())) == 1
    assert ct[1] == min(k, 128) and set(row[1, :ct[1]].tolist()) <= set(info["lose_b"].tolist())
    assert ct[3] == 6


def test_k50_is_the_prefix_of_k128(merge_corpus):
    index, info = merge_corpus
    queries = planted_queries(info)
    big, small = run(index, queries, 128), run(index, queries, 50)
    assert np.array_equal(big[0][:, :50], small[0]) and np.array_equal(big[1][:, :50], small[1])
    assert np.array_equal(np.minimum(big[2], 50), small[2])


@pytest.mark.parametrize("k", [128, 100])
def test_a_query_alone_equals_number_63_of_64(merge_corpus, k):
    index, info = merge_corpus
    rng = np.random.default_rng(5)
    bg = np.asarray(info["bg"])
    print(f"merge: k={k}: {merge_rounds(info['n'], k)} round(s)")
    for last_query in (q(info["b"], info["c"], info["e"], *bg[10:40]), q(info["f"], info["d"])):
        others = [q(*rng.choice(bg, size=int(rng.integers(1, 9)), replace=False)) for _ in range(63)]
        others[5] = q()                                                   # an empty query among them
        others[40] = q(info["a"])
        alone = run(index, [last_query], k)
        batch = run(index, others + [last_query], k)
        assert batch[2][5] == 0
        for a, b in zip(alone, batch):
            assert np.array_equal(a[0], b[63])


@pytest.mark.parametrize("n", [39 * R, 39 * R + 1, 40 * R])
def test_merge_round_boundary(gpu, n):
    """k = 128 takes 39 lists a round: exactly one full round; a second round of one range that holds one row; a second
    round of one full range."""
    k, ranges, last = 128, math.ceil(n / R), n - 1
    assert merge_rounds(n, k) == (1 if n == 39 * R else 2)
    print(f"merge: {n} rows = {ranges} ranges, k={k}: {MERGE_KEYS // k} lists a round, {merge_rounds(n, k)} round(s)")
    rng = np.random.default_rng(n)
    c = Corpus(n)
    edges = np.array(sorted({p for r in range(0, n, R) for p in (r, min(r + R, n) - 1)}))
    t_edge = c.term(edges, 2)
    t_last = c.term([last], 3)
    losers = window(rng, 0, 1000, 128)
    t_carry = c.term(np.concatenate([losers, [last]]), np.concatenate([np.ones(128, int), [7]]))
    t_rand = c.term(np.unique(rng.integers(0, n, size=300)), 1)
    ftf = 1 + np.arange(n) % 3
    ftf[edges] = 1
    ftf[losers] = 1
    t_all = c.term(np.arange(n), ftf)
    ids = np.arange(n, dtype=np.int64) * 2 + 1
    index = c.index(ids)
    try:
        got, bits, ct = run(index, [q(t_edge), q(t_last), q(t_carry), q(t_rand), q(t_all),
                                    q(t_edge, t_last, t_carry, t_rand, t_all), q()], k)
        assert ct[0] == min(k, edges.size) and set(got[0, :ct[0]].tolist()) <= set(ids[edges].tolist())
        assert ct[1] == 1 and got[1, 0] == ids[last]
        assert ct[2] == k and got[2, 0] == ids[last], "the last row outscores every carried key"
        assert set(got[2, 1:].tolist()) < set(ids[losers].tolist())
        assert ct[4] == k and len(set(bits[4].tolist())) == 1 and ct[6] == 0
        only_last_range = np.zeros(n, dtype=bool)
        only_last_range[(ranges - 1) * R:] = True
        got, _, ct = run(index, [q(t_all), q(t_carry), q(t_edge)], k, only_last_range)
        assert ct[0] == min(k, n - (ranges - 1) * R) and ct[1] == 1 and got[1, 0] == ids[last]
        assert ct[2] == (1 if n == 39 * R + 1 else 2)
    finally:
        index.close()


# ---- the score kernel's rounds of 256 terms ----------------------------------------------------------------------

G0, G1, G2, G3, G4 = range(0, 256), range(256, 301), range(301, 557), range(557, 813), range(813, 831)


@pytest.fixture(scope="module")
def rounds_corpus(gpu):
    """4 ranges.  Terms 0-255 post in ranges 0-1 only, 301-556 in range 2 only, 557-812 in range 3 only, 813-830 in
    ranges 2-3, 256-300 anywhere."""
    n = 4 * R
    rng = np.random.default_rng(88)
    c = Corpus(n)
    for group, lo, hi in ((G0, 0, 2 * R), (G1, 0, n), (G2, 2 * R, 3 * R), (G3, 3 * R, n), (G4, 2 * R, n)):
        for _ in group:
            p = lo + np.unique(rng.integers(0, hi - lo, size=int(rng.integers(100, 1500))))
            c.term(p, rng.integers(1, 7, size=p.size))
    index = c.index(np.arange(n, dtype=np.int64) * 7 + 3)
    yield index
    index.close()


def test_term_rounds_with_a_late_first_hit(rounds_corpus):
    index = rounds_corpus
    post_ptr, post_pos, _ = index.host_csr()

    def rows_of(terms):
        return set(np.concatenate([post_pos[post_ptr[t]:post_ptr[t + 1]] for t in terms]).tolist())

    queries = {
        "255": q(*G0[:255]),                          # one round; ranges 2-3 untouched
        "256": q(*G0),                                # exactly one full round
        "257": q(*G0, 813),                           # ranges 0-1: round one, then idle; ranges 2-3: first touched in round two
        "257 anywhere": q(*G0, 256),                  # round two reaches ranges 0-1 again and ranges 2-3 for the first time
        "512": q(*G0, *G2),                           # round two is range 2's; range 3 is never touched
        "513 one and three": q(*G2, *G3, 813),        # range 2: rounds one and three, idle in two; range 3: two and three
        "513 first hit in three": q(*G0, *G2, 557),   # range 3 idle for two rounds
        "513 anywhere": q(*G0, 256, *G2),               # round two: term 256 in every range; round three: one term
        "one": q(400),
    }
    assert [len(queries[name][0]) for name in list(queries)[:8]] == [255, 256, 257, 257, 512, 513, 513, 513]
    for k in (128, 10):
        ids, _, ct = run(index, list(queries.values()), k)
        row = (ids - 3) // 7
        assert np.all(ct[:8] == k)
        assert np.all(row[0] < 2 * R) and np.all(row[1] < 2 * R), "ranges 2-3 hold no term of these queries"
        assert set(row[2][row[2] >= 2 * R].tolist()) <= rows_of([813])
        assert np.all(row[4] < 3 * R) and np.all(row[5] >= 2 * R)
        assert set(row[6][row[6] >= 3 * R].tolist()) <= rows_of([557])
    # every range's list on its own: a mask that leaves one range (ranges untouched by the query report nothing)
    for rg in range(4):
        only = np.zeros(4 * R, dtype=bool)
        only[rg * R:(rg + 1) * R] = True
        _, _, ct = run(index, list(queries.values()), 128, only, what=f"range {rg} only")
        want = {0: [1, 1, 1, 1, 1, 0, 1, 1, 0], 1: [1, 1, 1, 1, 1, 0, 1, 1, 0], 2: [0, 0, 1, 1, 1, 1, 1, 1, 1],
                3: [0, 0, 1, 1, 0, 1, 1, 1, 0]}[rg]
        assert (ct > 0).astype(int).tolist() == want, (rg, ct)
    # the batch does not matter: one query alone
    alone = run(index, [queries["513 one and three"]], 128)
    batch = run(index, list(queries.values()), 128)
    assert all(np.array_equal(a[0], b[5]) for a, b in zip(alone, batch))


# ---- the selection inside a range --------------------------------------------------------------------------------

COUNTS = (1, 2, 15, 16, 17, 18, 127, 128, 129)


@pytest.fixture(scope="module")
def select_corpus(gpu):
    """2 * R + 9 rows, every row of length 12 (a pad term evens the rows out): bits depend on tf alone."""
    n = 2 * R + 9
    rng = np.random.default_rng(99)
    c = Corpus(n)
    t = {"all": c.term(np.arange(n), 1), "range1": c.term(np.arange(R, 2 * R), 1)}
    t["m"] = {m: c.term(window(rng, 0, 100 + 200 * i, m, 200), rng.integers(1, 6, size=m)) for i, m in enumerate(COUNTS)}
    high, low = window(rng, 0, 4000, 10, 500), window(rng, 0, 4500, 300, 500)
    t["levels"] = c.term(np.concatenate([high, low]), np.concatenate([np.full(10, 3), np.ones(300, int)]))
    spots = np.array([0, 15, 16, R - 1, R + 8, 2 * R - 1, 2 * R + 8])
    others = np.concatenate([window(rng, 0, 6000, 100), [2 * R + 1, 2 * R + 3]])
    wpos = np.sort(np.concatenate([spots, others]))
    t["w"] = c.term(wpos, np.where(np.isin(wpos, spots), 4, 1))
    sums = c.row_sums()
    assert sums.max() <= 11
    c.term(np.arange(n), 12 - sums)
    index = c.index(np.arange(n, dtype=np.int64) + 1000)
    assert np.all(index.doc_len == 12)
    yield index, dict(t, n=n, high=high, low=low, spots=spots)
    index.close()


@pytest.mark.parametrize("k", [1, 16, 17, 128])
def test_selection_inside_a_range(select_corpus, k):
    index, t = select_corpus
    names = ["range1", "levels", "spots"] + [m for m in (k - 1, k, k + 1) if m > 0]
    queries = [q(t["range1"]), q(t["levels"]), q(t["w"])] + [q(t["m"][m]) for m in names[3:]]
    ids, bits, ct = run(index, queries, k)
    row = ids - 1000
    # a whole range on equal bits: the threshold falls into the 14 position bits, the lowest positions win
    assert ct[0] == k and np.array_equal(row[0], R + np.arange(k)) and len(set(bits[0].tolist())) == 1
    # two levels that straddle k (10 rows above, 300 below)
    want = np.concatenate([t["high"], t["low"]])[:k]
    assert ct[1] == k and np.array_equal(row[1], want)
    # winners at the first and last positions of the threads' groups of 16 and of the ranges
    assert ct[2] == min(k, 109) and np.array_equal(row[2, :min(k, 7)], t["spots"][:k])
    assert len(set(bits[2, :min(k, 7)].tolist())) == 1
    # k - 1, k and k + 1 touched rows
    for i, m in enumerate(names[3:]):
        assert ct[3 + i] == min(m, k), (m, k)


def test_selection_under_masks(select_corpus):
    index, t = select_corpus
    n = t["n"]
    masks = np.ones((8, n), dtype=bool)
    masks[0, [0, 15, 16, 31, 32]] = False                    # the edges of a thread's 16 rows and of a mask word
    masks[1, :] = False
    masks[1, 2 * R:] = True                                  # the 9 rows of the partial last word
    masks[2, :R + 16] = False
    masks[3, :] = False
    masks[3, [5, R + 3]] = True                              # fewer than k rows
    masks[4, :] = False
    masks[6, ::2] = False
    masks[7, :R - 1] = False
    masks[7, R + 1:2 * R + 8] = False                        # last row of range 0, first of range 1, last row of all
    packed = DenseIndex.pack_mask(masks)
    packed[1, 2 * R // 8 + 1] |= 0xFE                        # bits behind the last row are set: they name no row
    packed[1, 2 * R // 8 + 2:] = 0xFF
    packed[5, 2 * R // 8 + 1:] = 0xFF
    for k in (1, 16, 17, 128):
        ids, bits, ct = run(index, [q(t["all"])] * 8, k, masks, packed)
        row = ids - 1000
        for i in range(8):
            want = np.flatnonzero(masks[i])[:k]
            assert ct[i] == want.size and np.array_equal(row[i, :ct[i]], want), (k, i)
            assert len(set(bits[i, :ct[i]].tolist())) <= 1
        assert ct.tolist() == [k, min(k, 9), k, min(k, 2), 0, k, k, min(k, 3)]
        # masks over scores that differ, per query and shared
        queries = [q(t["levels"]), q(t["w"]), q(t["m"][129]), q(t["range1"]), q(t["m"][17], t["levels"]),
                   q(t["all"], t["w"]), q(t["m"][128]), q(t["w"])]
        run(index, queries, k, masks, packed)
        run(index, queries, k, masks[6])
        shared = np.ones(n, dtype=bool)
        shared[t["high"][::2]] = False
        shared[t["spots"][[0, 3, 6]]] = False
        ids, _, ct = run(index, queries, k, shared)
        assert np.array_equal(ids[1, :min(k, 4)] - 1000, t["spots"][[1, 2, 4, 5]][:k])
        want = np.concatenate([t["high"][1::2], t["low"]])[:k]
        assert np.array_equal(ids[0] - 1000, want)


# ---- values, straight through the C ABI ------------------------------------------------------------------------

def lane_host(lib, dev, n, n_terms, avgdl, queries, k, d_ids=None, d_mask=None, mask_stride=0):
    q_ptr = np.zeros(len(queries) + 1, dtype=np.int32)
    q_ptr[1:] = np.cumsum([len(t) for t, _ in queries])
    terms = np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int32) for t, _ in queries]))
    w = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float32) for _, x in queries]))
    nq = len(queries)
    out_ids = torch.empty(nq, k, dtype=torch.int64, device=DEV)
    out_sc = torch.empty(nq, k, dtype=torch.float32, device=DEV)
    out_ct = torch.empty(nq, dtype=torch.int32, device=DEV)
    nbytes = lib.crag_bm25_scratch_bytes(n, nq, k)
    assert nbytes > 0
    scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=DEV)
    slot = lib.crag_upload_slot_create()
    assert slot
    try:
        rc = lib.crag_bm25_lane_host(dev["post_ptr"].data_ptr(), dev["post_pos"].data_ptr(), dev["post_tf"].data_ptr(),
                                     dev["doc_len"].data_ptr(), None if d_ids is None else d_ids.data_ptr(), n, n_terms,
                                     ctypes.c_float(avgdl), q_ptr.ctypes.data, terms.ctypes.data, w.ctypes.data, nq, k,
                                     None if d_mask is None else d_mask.data_ptr(), mask_stride, slot, scratch.data_ptr(), nbytes,
                                     out_ids.data_ptr(), out_sc.data_ptr(), out_ct.data_ptr(), None)
        assert rc == 0, _native.last_error()
    finally:
        torch.cuda.synchronize()
        lib.crag_upload_slot_destroy(slot)
    return out_ids.cpu().numpy(), out_sc.cpu().numpy().view(np.uint32), out_ct.cpu().numpy()


def test_extreme_values_through_the_c_abi(gpu):
    """tf 1 and 65 535; dl 0, 2^24 + 1 (not an fp32) and 2^31 - 1; weights 2^-40 and 2^40; ids NULL and above 2^40;
    rows with the same (tf..., dl) in three ranges."""
    n, n_terms, avgdl = 2 * R + 3, 6, 37.5
    rng = np.random.default_rng(123)
    doc_len = rng.integers(0, 200, size=n)                   # many short lengths: every rounding of the chain shows
    extreme = rng.random(n) < 0.25
    doc_len[extreme] = rng.choice(np.array([0, 1, 2 ** 24 + 1, 2 ** 31 - 1]), size=int(extreme.sum()))
    doc_len = doc_len.astype(np.int32)
    twins = np.array([37, R + 4111, 2 * R + 2])
    doc_len[twins] = 2 ** 24 + 1
    fixed = np.array([1, 65535, 2, 65535, 1, 300])
    pos_l, tf_l = [], []
    for term in range(n_terms):
        p = np.unique(np.concatenate([rng.integers(0, n, size=400), twins, [0, R - 1, R, n - 1]]))
        tf = rng.choice(np.array([1, 2, 300, 65535]), size=p.size)
        tf[np.isin(p, twins)] = fixed[term]
        pos_l.append(p)
        tf_l.append(tf)
    post_ptr = np.zeros(n_terms + 1, dtype=np.int64)
    post_ptr[1:] = np.cumsum([p.size for p in pos_l])
    post_pos = np.concatenate(pos_l).astype(np.int32)
    post_tf = np.concatenate(tf_l).astype(np.uint16)
    ids = np.arange(n, dtype=np.int64) * 3 + 2 ** 40 + 5
    dev = {"post_ptr": torch.from_numpy(post_ptr).to(DEV), "post_pos": torch.from_numpy(post_pos).to(DEV),
           "post_tf": torch.from_numpy(post_tf.view(np.int16)).to(DEV), "doc_len": torch.from_numpy(doc_len).to(DEV)}
    d_ids = torch.from_numpy(ids).to(DEV)
    lo, hi = np.float32(2.0 ** -40), np.float32(2.0 ** 40)
    queries = [(np.array([0], np.int32), np.array([lo])), (np.array([1], np.int32), np.array([hi])),
               (np.arange(6, dtype=np.int32), np.array([0.7, 1.3, 2.9, 0.11, 5.5, 1.0], np.float32)),
               (np.array([2, 3], np.int32), np.array([lo, lo * 2])), (np.array([4, 5], np.int32), np.array([hi, hi / 2])),
               (np.array([0, 5], np.int32), np.array([lo, hi]))]
    only_twins = np.zeros(n, dtype=bool)
    only_twins[twins] = True
    for k in (128, 10):
        for eligible in (None, only_twins):
            d_mask = None if eligible is None else torch.from_numpy(DenseIndex.pack_mask(eligible)).to(DEV)
            by_pos = lane_host(gpu, dev, n, n_terms, avgdl, queries, k, None, d_mask)
            by_id = lane_host(gpu, dev, n, n_terms, avgdl, queries, k, d_ids, d_mask)
            for i, (terms, w) in enumerate(queries):
                for got, id_arg in ((by_pos, None), (by_id, ids)):
                    want = replay(post_ptr, post_pos, post_tf, doc_len, avgdl, terms, w, k, id_arg, eligible)
                    assert got[2][i] == want[2], (k, i)
                    assert np.array_equal(got[0][i], want[0]) and np.array_equal(got[1][i], want[1]), (k, i)
                assert np.all(np.isfinite(by_pos[1][i, :by_pos[2][i]].view(np.float32)))
                assert np.all(by_pos[1][i, :by_pos[2][i]].view(np.float32) > 0)
                if eligible is not None:      # the same (tf..., dl) in ranges 0, 1 and 2: the same bits, ascending
                    assert by_pos[2][i] == min(k, 3) and np.array_equal(by_pos[0][i, :3], twins)
                    assert np.array_equal(by_id[0][i, :3], ids[twins]) and len(set(by_pos[1][i, :3].tolist())) == 1


def test_every_row_of_two_ranges_bit_for_bit(gpu):
    """Only k rows of a query come back, and the best of them are the short rows.  Here per-query masks cut 2 * R + 3
    rows into windows of 128, so that at k = 128 every row's bits are returned and compared: one term (a single
    w * tf / (tf + x), all lengths and tf) and three terms (the sum in term order)."""
    n, n_terms, avgdl, k = 2 * R + 3, 3, float(np.float32(3000.7)), 128
    rng = np.random.default_rng(321)
    doc_len = rng.integers(0, 9000, size=n).astype(np.int32)     # dl / avgdl in [0, 3): sums that change the binade
    post_ptr = np.arange(n_terms + 1, dtype=np.int64) * n
    post_pos = np.tile(np.arange(n, dtype=np.int32), n_terms)
    post_tf = rng.integers(1, 40, size=n_terms * n)
    post_tf[rng.random(post_tf.size) < 0.02] = 65535
    post_tf = post_tf.astype(np.uint16)
    dev = {"post_ptr": torch.from_numpy(post_ptr).to(DEV), "post_pos": torch.from_numpy(post_pos).to(DEV),
           "post_tf": torch.from_numpy(post_tf.view(np.int16)).to(DEV), "doc_len": torch.from_numpy(doc_len).to(DEV)}
    windows = math.ceil(n / k)
    masks = np.zeros((windows, n), dtype=bool)
    for i in range(windows):
        masks[i, i * k:(i + 1) * k] = True
    seen = np.zeros(n, dtype=int)
    for query in ((np.array([1], np.int32), np.array([1.7], np.float32)),
                  (np.arange(3, dtype=np.int32), np.array([0.7, 1.3, 2.9], np.float32))):
        for w0 in range(0, windows, 64):
            el = masks[w0:w0 + 64]
            packed = DenseIndex.pack_mask(el)
            got = lane_host(gpu, dev, n, n_terms, avgdl, [query] * len(el), k, None, torch.from_numpy(packed).to(DEV),
                            packed.shape[-1])
            for i in range(len(el)):
                want = replay(post_ptr, post_pos, post_tf, doc_len, avgdl, *query, k, None, el[i])
                assert want[2] == int(el[i].sum()) and got[2][i] == want[2], (w0 + i)
                assert np.array_equal(got[0][i], want[0]) and np.array_equal(got[1][i], want[1]), (w0 + i)
                seen[got[0][i][:got[2][i]]] += 1
    assert np.all(seen == 2), "every row was returned once per query"
