"""Oracle of the BM25 lane's query clauses, written from the rule in include/crag_dense.h (crag_bm25_clause_masks_host),
not from the kernel: plain Python and numpy over each row's sequence of token ids.

A row passes a query iff its input mask bit is set, it holds every required term, no excluded term, every required
phrase and no excluded phrase.  A row holds the phrase t0 .. t(m-1) iff some position p exists with token t_i at p + i
for every i -- a sublist search of the row's own sequence, so a phrase never spans two rows and a term may repeat.
Positions at or above 65 535 are not indexed: a token there does not exist for a phrase.  Unknown tokens (None here): in a
required clause the query matches nothing, in an excluded clause the clause is dropped.  Kind 4 matches nothing.

A query is a list of (kind, term ids) with the kinds of the C ABI; `clauses_of` makes one from a ParsedQuery."""
import numpy as np

REQ_TERM, EXC_TERM, REQ_PHRASE, EXC_PHRASE, NOTHING = 0, 1, 2, 3, 4
WHERE_MAX = 65535


def clauses_of(parsed, vocab_get):
    """ParsedQuery -> [(kind, term ids)], an unknown token as None."""
    return [(kind, tuple(vocab_get(tok) for tok in toks)) for kind, toks in parsed.clauses]


def holds_phrase(seq, phrase):
    seq = np.asarray(seq)[:WHERE_MAX]               # (tokens at positions >= 65 535 are not indexed)
    m = len(phrase)
    starts = seq.size - m + 1
    if starts <= 0:
        return False
    ok = np.ones(starts, dtype=bool)
    for i, t in enumerate(phrase):
        ok &= seq[i:i + starts] == t
    return bool(ok.any())


class ClauseOracle:
    """rows: one sequence of token ids per row, in token order."""

    def __init__(self, rows):
        self.rows = [np.asarray(r, dtype=np.int64).reshape(-1) for r in rows]
        self.n = len(self.rows)
        lens = np.array([r.size for r in self.rows], dtype=np.int64)
        # the rows' sequences back to back, with every token's row and its position inside the row
        self._flat = np.concatenate(self.rows) if self.n else np.empty(0, dtype=np.int64)
        self._row_of = np.repeat(np.arange(self.n), lens)
        self._pos = np.arange(self._flat.size) - np.repeat(np.cumsum(lens) - lens, lens)

    def holds_term(self, t):
        """bool [N]: the rows that hold token t anywhere (a term clause does not look at positions)."""
        h = np.zeros(self.n, dtype=bool)
        h[self._row_of[self._flat == t]] = True
        return h

    def holds_phrase_rows(self, phrase):
        """bool [N]: `holds_phrase` of every row at once -- the sublist search over the concatenated sequences, a match
        counting only where its first and last token lie in the same row and below position 65 535."""
        m = len(phrase)
        starts = self._flat.size - m + 1
        out = np.zeros(self.n, dtype=bool)
        if starts <= 0:
            return out
        ok = self._row_of[m - 1:m - 1 + starts] == self._row_of[:starts]
        ok &= self._pos[:starts] + (m - 1) < WHERE_MAX
        for i, t in enumerate(phrase):
            ok &= self._flat[i:i + starts] == t
        out[self._row_of[:starts][ok]] = True
        return out

    def passes(self, clauses, in_mask=None):
        """bool [N] of one query."""
        keep = np.ones(self.n, dtype=bool) if in_mask is None else np.asarray(in_mask, dtype=bool)[:self.n].copy()
        for kind, terms in clauses:
            unknown = any(t is None for t in terms)
            if kind == NOTHING or (unknown and kind in (REQ_TERM, REQ_PHRASE)):
                keep[:] = False
            elif unknown:
                continue                          # an excluded clause with an unknown token is dropped
            elif kind == REQ_TERM:
                keep &= self.holds_term(terms[0])
            elif kind == EXC_TERM:
                keep &= ~self.holds_term(terms[0])
            elif kind == REQ_PHRASE:
                keep &= self.holds_phrase_rows(terms)
            elif kind == EXC_PHRASE:
                keep &= ~self.holds_phrase_rows(terms)
            else:
                raise ValueError(f"kind {kind}")
        return keep

    def mask(self, queries, in_mask=None):
        """bool [nq, N].  in_mask: None, bool [N] (shared) or bool [nq, N]."""
        out = np.zeros((len(queries), self.n), dtype=bool)
        for q, clauses in enumerate(queries):
            im = None if in_mask is None else (in_mask[q] if np.ndim(in_mask) == 2 else in_mask)
            out[q] = self.passes(clauses, im)
        return out


def packed(mask, mask_stride):
    """bool [nq, N] -> the bytes of the output contract, uint8 [nq * mask_stride]: bit (i & 7) of byte i >> 3 of the
    query's run, the bits at or above N and the bytes up to mask_stride zero."""
    mask = np.asarray(mask, dtype=bool)
    bits = np.packbits(mask, axis=-1, bitorder="little")
    out = np.zeros((mask.shape[0], mask_stride), dtype=np.uint8)
    out[:, :bits.shape[1]] = bits
    return out.reshape(-1)


def arrays_from_rows(rows):
    """Token sequences -> the arguments of Bm25Index.from_arrays: row_ptr, row_terms (ascending inside a row), row_tf,
    pair_off, pair_where (the positions below 65 535 of every (row, term) pair, ascending)."""
    rows = [np.asarray(r, dtype=np.int64).reshape(-1) for r in rows]
    lens = np.array([r.size for r in rows], dtype=np.int64)
    flat = np.concatenate(rows) if rows else np.empty(0, dtype=np.int64)
    row_of = np.repeat(np.arange(len(rows)), lens)
    pos = np.arange(flat.size) - np.repeat(np.cumsum(lens) - lens, lens)
    order = np.lexsort((pos, flat, row_of))                     # by row, then term, then position
    flat, row_of, pos = flat[order], row_of[order], pos[order]
    head = np.ones(flat.size, dtype=bool)                       # the first token of every (row, term) pair
    head[1:] = (flat[1:] != flat[:-1]) | (row_of[1:] != row_of[:-1])
    pair = np.cumsum(head) - 1
    n_pairs = int(head.sum())
    row_ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(np.bincount(row_of[head], minlength=len(rows)), out=row_ptr[1:])
    indexed = pos < WHERE_MAX
    pair_off = np.zeros(n_pairs + 1, dtype=np.int64)
    np.cumsum(np.bincount(pair[indexed], minlength=n_pairs), out=pair_off[1:])
    return (row_ptr, flat[head].astype(np.int32), np.bincount(pair, minlength=n_pairs).astype(np.int64), pair_off,
            pos[indexed].astype(np.uint16))


# ---- the seeded random corpus the GPU tests share ---------------------------------------------------------------------
RANDOM_SEED = 20261021
RANDOM_ROWS, RANDOM_TERMS = 20000, 50


def random_corpus(seed=RANDOM_SEED, n_rows=RANDOM_ROWS, n_terms=RANDOM_TERMS):
    """Rows of 5-30 tokens over a Zipf vocabulary of n_terms term ids."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, n_terms + 1)
    p /= p.sum()
    lens = rng.integers(5, 31, size=n_rows)
    flat = rng.choice(n_terms, size=int(lens.sum()), p=p)
    return np.split(flat, np.cumsum(lens)[:-1])


def random_queries(rows, n_terms=RANDOM_TERMS, nq=64, seed=RANDOM_SEED + 1):
    """nq query strings over the decimal vocabulary ("17" is term 17) with 1-3 constraint clauses each, every kind in
    use, and one or two optional tokens.  Each query is built around one row that passes it: required terms and phrases
    are taken from that row, excluded ones are absent from it."""
    rng = np.random.default_rng(seed)
    out = []
    for q in range(nq):
        row = rows[int(rng.integers(len(rows)))]
        have = set(row.tolist())
        absent = [t for t in range(n_terms) if t not in have]
        items = []
        for c in range(1 + q % 3):
            kind = (q + c) % 4
            m = int(rng.integers(2, 4))
            at = int(rng.integers(0, row.size - m + 1))
            if kind == REQ_TERM:
                items.append(f"+{row[int(rng.integers(row.size))]}")
            elif kind == EXC_TERM:
                items.append(f"-{absent[int(rng.integers(len(absent)))]}")
            elif kind == REQ_PHRASE:
                items.append('"' + " ".join(str(t) for t in row[at:at + m]) + '"')
            else:
                ph = [int(t) for t in rng.choice(min(n_terms, 12), size=m)]      # frequent terms, in an order the row lacks
                while holds_phrase(row, ph):
                    ph = [int(t) for t in rng.choice(min(n_terms, 12), size=m)]
                items.append('-"' + " ".join(str(t) for t in ph) + '"')
        items += [str(int(t)) for t in rng.choice(row, size=1 + q % 2)]
        out.append(" ".join(items))
    return out
