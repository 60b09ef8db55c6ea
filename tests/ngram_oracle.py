"""CPU oracle of the character-trigram field, written from the prose of include/crag_dense.h (crag_ngram_extract) and
independent of cadence_rag_amd/ngram.py: the decoder is one regular expression over the bytes (the alternatives are the
valid sequences in the header's order; whatever none of them matches is one separator of one byte), the index is built
with dictionaries.  Also here: the hand-written rule goldens the host and the GPU tests share, the fixed corpus of the
fuzzy case, and the adapters that feed the gram CSR to tests/bm25_oracle.py (fp64) and tests/bm25_replay.py (fp32)."""
import re
from collections import Counter

import numpy as np

from bm25_oracle import Bm25Oracle

# a valid sequence: 1 byte | 2 bytes | 3 bytes | 4 bytes with a value <= 0x10FFFF (F0-F3 anything, F4 only below 90);
# overlong forms and surrogates are NOT excluded; any other byte alone
_SEQ = re.compile(rb"[\x00-\x7f]|[\xc0-\xdf][\x80-\xbf]|[\xe0-\xef][\x80-\xbf]{2}|[\xf0-\xf3][\x80-\xbf]{3}"
                  rb"|\xf4[\x80-\x8f][\x80-\xbf]{2}|([\x80-\xff])", re.DOTALL)
_PAYLOAD = {1: 0x7F, 2: 0x1F, 3: 0x0F, 4: 0x07}


def chars_of(data):
    """Per decoded unit of the row: the folded code point of a gram character, or None for a separator."""
    out = []
    for m in _SEQ.finditer(bytes(data)):
        seq = m.group(0)
        if m.group(1) is not None:
            out.append(None)
            continue
        cp = seq[0] & _PAYLOAD[len(seq)]
        for c in seq[1:]:
            cp = cp * 64 + (c & 0x3F)
        if ord("A") <= cp <= ord("Z"):
            cp += 32
        gram_char = cp >= 0x80 or chr(cp).isdigit() or "a" <= chr(cp) <= "z"
        out.append(cp if gram_char else None)
    return out


def key(a, b, c):
    return a * 2**42 + b * 2**21 + c


def keys_of(data):
    ch = chars_of(data)
    return [key(*ch[i:i + 3]) for i in range(len(ch) - 2) if None not in ch[i:i + 3]]


def csr_of(rows_bytes):
    """keys, post_ptr, post_pos, post_tf, doc_len of the rows' index, as ngram_csr_host returns them."""
    counts = [Counter(keys_of(r)) for r in rows_bytes]
    post = {}
    for r, c in enumerate(counts):
        for k, tf in c.items():
            post.setdefault(k, []).append((r, min(tf, 65535)))
    keys = sorted(post)
    post_ptr = np.zeros(len(keys) + 1, dtype=np.int64)
    pos, tf = [], []
    for t, k in enumerate(keys):
        post_ptr[t + 1] = post_ptr[t] + len(post[k])
        pos += [r for r, _ in post[k]]
        tf += [f for _, f in post[k]]
    return {"keys": np.asarray(keys, dtype=np.int64), "post_ptr": post_ptr, "post_pos": np.asarray(pos, dtype=np.int32),
            "post_tf": np.asarray(tf, dtype=np.uint16),
            "doc_len": np.asarray([sum(c.values()) for c in counts], dtype=np.int32).reshape(-1)}


def assert_csr_equal(got, want, what=""):
    """Element for element: keys, post_ptr, post_pos, post_tf, doc_len (and with them V and nnz)."""
    for name in ("keys", "post_ptr", "post_pos", "post_tf", "doc_len"):
        g, w = np.asarray(got[name]), np.asarray(want[name])
        assert g.dtype == w.dtype, f"{what}: {name} is {g.dtype}, expected {w.dtype}"
        assert g.shape == w.shape, f"{what}: {name} has {g.shape[0]} entries, expected {w.shape[0]}"
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{what}: {name}[{bad[0]}] = {g[bad[0]]}, expected {w[bad[0]]} ({bad.size} differ)"


class GramBm25Oracle(Bm25Oracle):
    """tests/bm25_oracle.py fed the gram CSR: its "tokens" are the decimal keys, a query is `as_query(bytes)`."""

    def __init__(self, rows_bytes, ids):
        csr = csr_of(rows_bytes)
        self.ids = np.asarray(ids, dtype=np.int64)
        self.n = len(rows_bytes)
        self.dl = csr["doc_len"].astype(np.float64)
        self.avgdl = float(self.dl.sum() / self.n) if self.n else 0.0
        ptr = csr["post_ptr"]
        self.post = {str(int(k)): (csr["post_pos"][ptr[t]:ptr[t + 1]].astype(np.int64),
                                   csr["post_tf"][ptr[t]:ptr[t + 1]].astype(np.float64))
                     for t, k in enumerate(csr["keys"])}

    @staticmethod
    def as_query(data):
        data = data.encode("utf-8", "replace") if isinstance(data, str) else data
        return " ".join(str(k) for k in keys_of(data))


class HostCsr:
    """What tests/bm25_replay.replay_index reads of an index, over a host CSR."""

    def __init__(self, csr, ids):
        self.csr, self.ids, self.doc_len = csr, np.asarray(ids, dtype=np.int64), csr["doc_len"]
        n = self.ids.size
        self.avgdl = float(np.float32(float(self.doc_len.sum(dtype=np.float64)) / n)) if n else 1.0

    def __len__(self):
        return int(self.ids.size)

    def host_csr(self):
        return self.csr["post_ptr"], self.csr["post_pos"], self.csr["post_tf"]


# ---- rule goldens, by hand: (row bytes, the grams as triples of code points) ------------------------------------------
A, B_, C, D, E, F, X, Y, Z = (ord(c) for c in "abcdefxyz")
EACUTE, EACUTE_UP, EURO, GRIN, TOP = 0xE9, 0xC9, 0x20AC, 0x1F600, 0x10FFFF
ABC, DEF = (A, B_, C), (D, E, F)
GOLDEN = [
    # sequences of 1, 2, 3 and 4 bytes mixed inside one gram
    (b"a\xc3\xa9\xe2\x82\xac\xf0\x9f\x98\x80", [(A, EACUTE, EURO), (EACUTE, EURO, GRIN)]),
    (b"\xf0\x9f\x98\x80\xe2\x82\xac\xc3\xa9a", [(GRIN, EURO, EACUTE), (EURO, EACUTE, A)]),
    # folding of A-Z only
    (b"AbZ", [(A, B_, Z)]),
    (b"\xc3\x89Xy", [(EACUTE_UP, X, Y)]),
    (b"\xc3\xa9Xy", [(EACUTE, X, Y)]),
    (b"a1B2", [(A, ord("1"), B_), (ord("1"), B_, ord("2"))]),
    # separators
    (b"ab cd", []),
    (b"abc_def", [ABC, DEF]),
    (b"abc-def", [ABC, DEF]),
    (b"ab\x00cd", []),
    (b"abc\x00def", [ABC, DEF]),
    (b" abc ", [ABC]),
    (b"a.b,c", []),
    # runs of 0, 1, 2, 3 and 4 characters
    (b"", []),
    (b" ", []),
    (b"a", []),
    (b"ab", []),
    (b"abc", [ABC]),
    (b"abcd", [ABC, (B_, C, D)]),
    (b"\xc3\xa9\xc3\xa9", []),
    (b"aaaa", [(A, A, A), (A, A, A)]),
    # a stray continuation
    (b"ab\x80cd", []),
    (b"abc\x80def", [ABC, DEF]),
    (b"\x80abc", [ABC]),
    (b"abc\xbf", [ABC]),
    (b"a\xc3\xa9\xa9bc", []),                      # the second A9 follows a complete sequence
    # a lead cut off by the row end, at each length
    (b"abc\xc3", [ABC]),
    (b"ab\xc3", []),
    (b"abc\xe2", [ABC]),
    (b"abc\xe2\x82", [ABC]),
    (b"abc\xf0", [ABC]),
    (b"abc\xf0\x9f", [ABC]),
    (b"abc\xf0\x9f\x98", [ABC]),
    (b"ab\xf0\x9f\x98", []),
    # a bad continuation in second, third and fourth place: the lead is one separator, decoding resumes behind it
    (b"\xc3abc", [ABC]),
    (b"ab\xc3cd", []),
    (b"\xe2abc", [ABC]),
    (b"\xe2\x82abc", [ABC]),
    (b"\xf0abc", [ABC]),
    (b"\xf0\x9fabc", [ABC]),
    (b"\xf0\x9f\x98abc", [ABC]),
    (b"ab\xf0\x9f\x98cd", []),
    (b"ab\xe2\xc3\xa9c", []),                      # E2 is malformed, C3 A9 behind it is not: a b | e-acute c
    (b"\xe2\xc3\xa9bc", [(EACUTE, B_, C)]),
    # above 0x10FFFF
    (b"ab\xf4\x90\x80\x80c", []),
    (b"abc\xf4\x90\x80\x80def", [ABC, DEF]),
    (b"ab\xf4\x8f\xbf\xbf", [(A, B_, TOP)]),
    (b"ab\xf5\x80\x80\x80", []),
    (b"ab\xf7\xbf\xbf\xbf", []),
    # F8-FF (each byte of the range is looped over in the test as well)
    (b"ab\xf8cd", []),
    (b"abc\xffdef", [ABC, DEF]),
    (b"abc\xfe", [ABC]),
    # what "not checked" means: an overlong 'A' folds like 'A', an overlong NUL separates, a surrogate is a character
    (b"\xc1\x81bc", [ABC]),
    (b"ab\xc0\x80c", []),
    (b"\xed\xa0\x80ab", [(0xD800, A, B_)]),
]

# ---- the fuzzy case ---------------------------------------------------------------------------------------------------
FUZZY_ROWS = [
    "We deployed the kubernetes gateway on Friday.",
    "The gateway timeout was raised to thirty seconds.",
    "Kubernetes upgrade is planned for the next sprint.",
    "Action item: file ticket ABC-12345 for the outage.",
    "abc 12345 was mentioned first, abc12345 later.",
    "Let's roll back version 1.2.3 tonight.",
    "We saw ECONNRESET in the api proxy.",
    "Budget review moved to Tuesday.",
]
FUZZY_QUERY, FUZZY_ROW = "kubernets gatewy", 0


def random_rows(seed, n_rows, max_pieces=120):
    """Seeded rows over an alphabet that mixes the four widths, separators and about 2 % malformed pieces."""
    rng = np.random.default_rng(seed)
    good = ([c.encode() for c in "abcdeABC0123"] + [b" ", b" ", b" ", b"-", b"_", b"\x00", b"."]
            + ["é".encode(), "É".encode(), "ß".encode(), "Ж".encode()] + ["€".encode(), "中".encode(), "文".encode()]
            + ["😀".encode(), "𝄞".encode(), b"\xf4\x8f\xbf\xbf"])
    bad = [b"\x80", b"\xbf", b"\xc3", b"\xe2\x82", b"\xe2", b"\xf0\x9f", b"\xf0\x9f\x98", b"\xff", b"\xf8",
           b"\xf4\x90\x80\x80", b"\xf5"]
    weight = 1.0 / (1 + (np.arange(len(good)) * 7) % len(good))     # skewed, so that grams repeat inside a row
    weight /= weight.sum()
    rows = []
    for _ in range(n_rows):
        n = int(rng.integers(0, max_pieces + 1))
        pick_bad = rng.random(n) < 0.02
        gi, bi = rng.choice(len(good), n, p=weight), rng.integers(0, len(bad), n)
        rows.append(b"".join(bad[bi[j]] if pick_bad[j] else good[gi[j]] for j in range(n)))
    return rows
