"""The character-trigram rule on the host (cadence_rag_amd/ngram.py) against hand-written goldens and the independent
oracle of tests/ngram_oracle.py; query weights against an fp64 restatement; the fuzzy property of the field through
tests/bm25_oracle.py fed the gram CSR."""
import re
from pathlib import Path

import numpy as np
import pytest

from bm25_oracle import Bm25Oracle
from cadence_rag_amd import _native, ngram
from ngram_oracle import (FUZZY_QUERY, FUZZY_ROW, FUZZY_ROWS, GOLDEN, GramBm25Oracle, assert_csr_equal, csr_of, key,
                          keys_of, random_rows)


@pytest.mark.parametrize("case", range(len(GOLDEN)))
def test_rule_goldens(case):
    data, grams = GOLDEN[case]
    want = [key(*g) for g in grams]
    assert ngram.ngram_keys_host(data) == want, data
    assert keys_of(data) == want, data            # the oracle is held to the same goldens


def test_every_byte_f8_to_ff_is_a_separator():
    for b in range(0xF8, 0x100):
        assert ngram.ngram_keys_host(b"ab" + bytes([b]) + b"c") == []
        assert ngram.ngram_keys_host(b"abc" + bytes([b]) + b"\x80\x80\x80\x80") == [key(97, 98, 99)]


def test_key_is_exact_and_below_2_63():
    top = ngram.ngram_keys_host(b"\xf4\x8f\xbf\xbf" * 3)
    assert top == [0x10FFFF << 42 | 0x10FFFF << 21 | 0x10FFFF] and top[0] < ngram.NO_KEY == 2**63 - 1
    assert ngram.ngram_keys_host(b"\x30\x30\x30") == [0x30 << 42 | 0x30 << 21 | 0x30]


def test_ngram_keys_encodes_utf8_and_replaces_lone_surrogates():
    assert ngram.ngram_keys("Aé€😀") == ngram.ngram_keys_host("aé€😀".encode())
    assert ngram.ngram_keys("ab\ud800c") == []                      # '?' is a separator
    assert ngram.ngram_keys("") == [] and ngram.ngram_keys(None) == []


def test_tile_constant_is_the_headers():
    header = (Path(__file__).resolve().parent.parent / "include" / "crag_dense.h").read_text()
    assert int(re.search(r"#define CRAG_NGRAM_TILE (\d+)", header).group(1)) == ngram.TILE_BYTES == _native.CRAG_NGRAM_TILE


def test_csr_host_agrees_with_the_independent_oracle():
    assert_csr_equal(ngram.ngram_csr_host([]), csr_of([]), "no rows")
    assert_csr_equal(ngram.ngram_csr_host([b"", b"ab"]), csr_of([b"", b"ab"]), "no grams")
    assert_csr_equal(ngram.ngram_csr_host([g[0] for g in GOLDEN]), csr_of([g[0] for g in GOLDEN]), "goldens")
    rows = random_rows(11, 400)
    got = ngram.ngram_csr_host(rows)
    assert_csr_equal(got, csr_of(rows), "random rows")
    assert got["keys"].size > 100 and got["post_tf"].max() > 1 and np.diff(got["post_ptr"]).max() > 1
    assert np.all(np.diff(got["keys"]) > 0)
    sat = [b"a" * 65540, b"a" * 65537, b"a" * 65536]
    got = ngram.ngram_csr_host(sat)
    assert got["post_tf"].tolist() == [65535, 65535, 65534] and got["doc_len"].tolist() == [65538, 65535, 65534]


def test_query_terms_weights_match_an_fp64_restatement():
    rows = random_rows(12, 300)
    csr = ngram.ngram_csr_host(rows)
    df = np.diff(csr["post_ptr"])
    queries = [rows[5][:40], b"abc abc abcd \xe2\x82\xacab zzzzqq", "É0a1b2 cab", b"", b"ab"]
    q_ptr, terms, weights = ngram.query_terms_host(csr["keys"], df, len(rows), queries)
    assert q_ptr.dtype == np.int32 and terms.dtype == np.int32 and weights.dtype == np.float32 and q_ptr[0] == 0
    index_of = {int(k): t for t, k in enumerate(csr["keys"])}
    for q, text in enumerate(queries):
        data = text.encode() if isinstance(text, str) else text
        qtf = {}
        for k in keys_of(data):
            if k in index_of:
                qtf[index_of[k]] = qtf.get(index_of[k], 0) + 1
        want_terms = sorted(qtf)
        got = slice(q_ptr[q], q_ptr[q + 1])
        assert terms[got].tolist() == want_terms
        want_w = [qtf[t] * np.log(1.0 + (len(rows) - float(df[t]) + 0.5) / (float(df[t]) + 0.5)) * 2.2 for t in want_terms]
        assert np.array_equal(weights[got], np.asarray(want_w, dtype=np.float64).astype(np.float32))
    assert q_ptr[2] - q_ptr[1] > 0 and q_ptr[4] == q_ptr[3] == q_ptr[5]
    assert any(c > 1 for c in np.unique(keys_of(queries[1]), return_counts=True)[1])    # a qtf above 1 is in play


def test_fuzzy_query_finds_the_row_the_word_lane_misses():
    ids = np.arange(len(FUZZY_ROWS), dtype=np.int64) + 10
    words = Bm25Oracle(FUZZY_ROWS, ids)
    assert words.topk(FUZZY_QUERY, 5)[2] == 0                        # neither token is in the vocabulary
    grams = GramBm25Oracle([t.encode() for t in FUZZY_ROWS], ids)
    got_ids, got_scores, count = grams.topk(GramBm25Oracle.as_query(FUZZY_QUERY), 5)
    assert count >= 2 and got_ids[0] == ids[FUZZY_ROW] and got_scores[0] > got_scores[1]
    # a ticket id spoken without its dash finds both spellings
    got_ids, _, count = grams.topk(GramBm25Oracle.as_query("ABC12345"), 5)
    assert {13, 14} <= set(got_ids[:count].tolist())
