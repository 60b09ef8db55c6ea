"""Oracle of the BM25 lane's prefix and fuzzy items, written from the rule in include/crag_dense.h (crag_bm25_expand_host,
crag_bm25_group_masks_host), not from the kernels: plain Python over `str`, numpy only for the masks.

  read(text)            the parser's reading with `expand`: (clauses, bag, text, expansions)
  matches(...)          the terms a pattern stands for, in the kept order, cut at 64, and the number of all matches
  group_mask(...)       in AND (every required group: OR of its terms' rows) AND NOT (OR of the excluded groups' rows)
  weights(...)          the fp64 weights of a query, rounded once to fp32
Kinds: 0 prefix, 1 fuzzy with distance 1, 2 fuzzy with distance 2.  Roles: 0 optional, 1 required, 2 excluded."""
import math

import numpy as np

PREFIX, FUZZY1, FUZZY2 = 0, 1, 2
OPTIONAL, REQUIRED, EXCLUDED = 0, 1, 2
REQ_TERM, EXC_TERM, REQ_PHRASE, EXC_PHRASE = 0, 1, 2, 3
KEEP = 64
MAX_ITEMS, MAX_CLAUSES, MAX_PHRASE = 8, 16, 8
K1 = 1.2


class TooMuch(ValueError):
    """Over a limit of the syntax."""


def tokens(text):
    """Maximal runs of alphanumeric characters, lower-cased; a token above 255 UTF-8 bytes is dropped."""
    out, run = [], []
    for ch in (text or "") + " ":
        if ch.isalnum():
            run.append(ch)
        elif run:
            tok = "".join(run).lower()
            if len(tok.encode("utf-8")) <= 255:
                out.append(tok)
            run = []
    return out


def items(text):
    """(prefix, quoted, raw) of every item: whitespace separates outside quotes, a quote opens a quoted item and ends an
    unquoted one, an unclosed quote runs to the end; a prefix stands at the start or behind whitespace, touching its item."""
    s, i, out = text or "", 0, []
    while i < len(s):
        if s[i].isspace():
            i += 1
            continue
        prefix = ""
        if s[i] in "+-" and (i == 0 or s[i - 1].isspace()) and i + 1 < len(s) and not s[i + 1].isspace():
            prefix, i = s[i], i + 1
        if s[i] == '"':
            j = s.find('"', i + 1)
            j = len(s) if j < 0 else j
            out.append((prefix, True, s[i + 1:j]))
            i = j + 1
        else:
            j = i
            while j < len(s) and not s[j].isspace() and s[j] != '"':
                j += 1
            out.append((prefix, False, s[i:j]))
            i = j
    return out


def operator_of(raw):
    """(front, kind) of an unquoted item that ends in one operator whose front is exactly one token, else None."""
    for op, kind in (("~1", FUZZY1), ("~2", FUZZY2), ("~", FUZZY1), ("*", PREFIX)):
        if raw.endswith(op):
            front = raw[:len(raw) - len(op)]
            return (front, kind) if len(tokens(front)) == 1 else None
    return None


def read(text, expand=True):
    """-> (clauses [(kind, tokens)], bag [token], text, expansions [(role, kind, token)]).  expand False: no operator is
    syntax (the reading of crag_bm25_clause_masks_host)."""
    clauses, bag, kept, exp = [], [], [], []
    constrained = 0
    for prefix, quoted, raw in items(text):
        role = EXCLUDED if prefix == "-" else REQUIRED if prefix == "+" else OPTIONAL
        op = None if quoted or not expand else operator_of(raw)
        if op is not None:
            exp.append((role, op[1], tokens(op[0])[0]))
            constrained += role != OPTIONAL
            if role != EXCLUDED:
                kept.append(op[0].strip())
        else:
            toks = tokens(raw)
            if not toks:
                continue
            if quoted and len(toks) > 1:
                if len(toks) > MAX_PHRASE:
                    raise TooMuch("phrase")
                clauses.append((EXC_PHRASE if role == EXCLUDED else REQ_PHRASE, tuple(toks)))
            elif role == EXCLUDED:
                clauses += [(EXC_TERM, (t,)) for t in toks]
            elif quoted or role == REQUIRED:
                clauses += [(REQ_TERM, (t,)) for t in toks]
            if role != EXCLUDED:
                bag += toks
                kept.append(raw.strip())
        if len(exp) > MAX_ITEMS or len(clauses) + constrained > MAX_CLAUSES:
            raise TooMuch("items or clauses")
    return clauses, bag, " ".join(kept), exp


def levenshtein(a, b):
    """Plain edit distance over code points: insertion, deletion, substitution cost 1 each."""
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def distance(kind, pattern, term):
    """The match's distance, or None."""
    if kind == PREFIX:
        return 0 if term.startswith(pattern) else None
    if abs(len(term) - len(pattern)) > kind:
        return None
    d = levenshtein(pattern, term)
    return d if d <= kind else None


def matches(terms, df, kind, pattern):
    """terms: the vocabulary in term-id order; df [V].  -> (kept ids, their distances, number of all matches)."""
    hits = []
    for t, term in enumerate(terms):
        d = distance(kind, pattern, term)
        if d is not None:
            hits.append((d, -int(df[t]), t))
    hits.sort()
    return [t for _, _, t in hits[:KEEP]], [d for d, _, _ in hits[:KEEP]], len(hits)


def group_mask(holds, groups, in_mask=None):
    """holds(t) -> bool [N], the rows that hold term t; groups: [(kind 0 required-any / 1 excluded-any, term ids)]."""
    keep = None if in_mask is None else np.asarray(in_mask, dtype=bool).copy()
    for kind, ids in groups:
        any_of = None
        for t in ids:
            any_of = holds(t) if any_of is None else any_of | holds(t)
        if keep is None:
            keep = np.ones_like(holds(0) if any_of is None else any_of, dtype=bool)
        if any_of is None:
            if kind == 0:
                keep[:] = False           # an empty required group matches nothing
            continue                      # an empty excluded group has no effect
        keep &= any_of if kind == 0 else ~any_of
    return keep


def idf_weight(n, df):
    return math.log(1.0 + (n - df + 0.5) / (df + 0.5)) * (K1 + 1.0)


def weights(n_rows, df, bag_ids, item_matches):
    """bag_ids: the term ids of the plain bag's known tokens, with repeats; item_matches: per NON-EXCLUDED expanding item,
    in item order, (kept ids, distances).  -> (term ids ascending, fp32 weights)."""
    w = {}
    for t in sorted(set(bag_ids)):
        w[t] = float(bag_ids.count(t)) * math.log(1.0 + (n_rows - df[t] + 0.5) / (df[t] + 0.5)) * (K1 + 1.0)
    for ids, dist in item_matches:
        if not len(ids):
            continue
        base = idf_weight(float(n_rows), float(max(int(df[t]) for t in ids)))
        for t, d in zip(ids, dist):
            w[t] = w.get(t, 0.0) + base * 2.0 ** (-d)
    order = sorted(w)
    return np.asarray(order, dtype=np.int32), np.asarray([w[t] for t in order], dtype=np.float64).astype(np.float32)


def query_plan(text, terms, df, n_rows, vocab_get):
    """Everything the rule says about one query over a vocabulary: the plain clauses (kind, term ids or None), the any-of
    groups, and the scored terms with their weights."""
    clauses, bag, _, exp = read(text)
    found = [matches(terms, df, kind, tok) for _, kind, tok in exp]
    groups = []
    for (role, _, _), (ids, _, _) in zip(exp, found):
        if role == REQUIRED:
            groups.append((0, ids))
        elif role == EXCLUDED and ids:
            groups.append((1, ids))
    bag_ids = [vocab_get(t) for t in bag if vocab_get(t) is not None]
    scored = [(ids, dist) for (role, _, _), (ids, dist, _) in zip(exp, found) if role != EXCLUDED]
    ids, w = weights(n_rows, df, bag_ids, scored)
    return [(kind, tuple(vocab_get(t) for t in toks)) for kind, toks in clauses], groups, ids, w


# ---- the matching rule on cases written out by hand: (kind, pattern, term, distance or None) ---------------------------
LONG = "a" * 255
GOLDENS = [
    (FUZZY1, "abcdef", "abcdef", 0), (FUZZY2, "abcdef", "abcdef", 0), (PREFIX, "abcdef", "abcdef", 0),
    (FUZZY1, "abcdef", "abcdex", 1), (FUZZY1, "abcdef", "xbcdef", 1),          # an edit at the last / first code point
    (FUZZY1, "abcdef", "xbcdey", None), (FUZZY2, "abcdef", "xbcdey", 2),        # distance d + 1 / exactly d
    (FUZZY2, "abcdef", "xbcyez", None),                                         # 3
    (FUZZY1, "abcdef", "abdcef", None), (FUZZY2, "abcdef", "abdcef", 2),        # a transposition costs 2
    (FUZZY1, "abc", "abcd", 1), (FUZZY1, "abc", "abcde", None),                 # length difference d / d + 1
    (FUZZY2, "abc", "abcde", 2), (FUZZY2, "abc", "abcdef", None),
    (FUZZY1, "abcd", "bcd", 1), (FUZZY2, "abcd", "cd", 2), (FUZZY2, "abcd", "d", None),
    (FUZZY1, "kubernets", "kubernetes", 1), (FUZZY2, "kubernets", "kubernetes", 1),
    (FUZZY1, "naive", "na\u00efve", 1), (FUZZY1, "na\u00efve", "naive", 1),       # 1 byte against 2 bytes
    (FUZZY2, "gr\u00f6\u00dfe", "gr\u00f6sse", 2), (FUZZY1, "gr\u00f6\u00dfe", "gr\u00f6sse", None),
    (FUZZY1, "\u6771\u4eac\u30bf\u30ef\u30fc", "\u6771\u4eac\u30bf\u30ef", 1),   # 3-byte code points
    (FUZZY1, "\u6771\u4eac\u30bf\u30ef\u30fc", "\u6771\u4eac\u30bf\u30fc\u30ef", None),
    (FUZZY2, "\u6771\u4eac\u30bf\u30ef\u30fc", "\u6771\u4eac\u30bf\u30fc\u30ef", 2),
    (FUZZY1, "a\U00010437b", "a\U00010437c", 1), (FUZZY1, "a\U00010437b", "ab", 1),   # a 4-byte code point; 4 bytes fewer
    (FUZZY1, "a\U00010437b", "a\U00010438b", 1), (PREFIX, "a\U00010437", "a\U00010437b", 0),
    (FUZZY1, "caf\u6771", "cafe", 1), (FUZZY1, "cafe", "caf\u6771", 1),          # byte lengths differ by 2, distance 1
    (FUZZY1, LONG, LONG[:-1] + "b", 1), (FUZZY2, LONG, "b" + LONG[1:-1] + "b", 2), (FUZZY1, LONG, "b" + LONG[1:-1] + "b", None),
    (PREFIX, LONG, LONG, 0), (PREFIX, LONG[:200], LONG, 0), (FUZZY1, LONG[:-1], LONG, 1),
    (PREFIX, "abcdefghij", "abc", None), (FUZZY1, "abcdefghij", "abc", None), (FUZZY2, "abcdefghij", "abc", None),
    (PREFIX, "deploy", "deploy", 0), (PREFIX, "deployx", "deploy", None), (PREFIX, "dep", "deploy", 0),
    (PREFIX, "dex", "deploy", None), (PREFIX, "gr", "gr\u00f6\u00dfe", 0), (PREFIX, "gr\u00f6", "gr\u00f6\u00dfe", 0),
    (PREFIX, "gro", "gr\u00f6\u00dfe", None), (PREFIX, "\u6771", "\u6771\u4eac\u30bf\u30ef\u30fc", 0),
    (PREFIX, "\u6772", "\u6771\u4eac\u30bf\u30ef\u30fc", None),              # the last byte of the code point differs
    (FUZZY2, "ab", "b", 1), (FUZZY2, "a", "bc", 2), (FUZZY1, "a", "b", 1), (FUZZY1, "a", "bc", None),
]
