"""The citation grammar on the host: soundness against answer.validate_citations by seeded random walks, liveness, the
accepted and refused texts of the specification, the token table of a byte-level BPE tokenizer, the caps, and
answer_question passing (or not passing) a grammar to its chat model."""
from __future__ import annotations

import random

import numpy as np
import pytest

import grammar_oracle as go
from cadence_rag_amd import answer, grammar, retrieve
from cadence_rag_amd.answer import AnswerRequest, validate_citations
from cadence_rag_amd.config import settings
from cadence_rag_amd.grammar import (ByteDfa, TokenGrammar, TokenTable, accepts, allowed_tokens_host, citation_grammar,
                                     next_state_host, walk)


@pytest.fixture(scope="module")
def dfa():
    return citation_grammar(go.IDS)


def _fuzz(dfa, alphabet, walks, seed, max_steps=80):
    """Random walks over `alphabet`, each finished by a shortest path to acceptance: the texts the validator refuses."""
    alive = go.alive_bytes(dfa, alphabet)
    finish = go.completions(dfa, alphabet)
    rng = random.Random(seed)
    failures = []
    for _ in range(walks):
        data, state = go.random_walk(dfa, alive, rng, rng.randrange(1, max_steps))
        data += finish[state]
        assert accepts(dfa, data)
        text = data.decode("utf-8", "replace")
        if text == answer.INSUFFICIENT:          # accepted as a whole reply: answer_question maps it to its own status
            continue
        if not validate_citations(text, go.IDS)["valid"]:
            failures.append(text)
    return failures


def test_soundness_fuzz_every_accepted_text_is_valid(dfa):
    """50 000 walks over the specification's alphabet: the cap is 0 failures."""
    failures = _fuzz(dfa, go.ALPHABET, 50_000, seed=20261019)
    assert not failures, failures[:5]


def test_soundness_fuzz_over_all_bytes(dfa):
    """The same over all 256 bytes (invalid UTF-8 decodes with replacement characters, as a tokenizer's decode does):
    the forbidden controls and the non-ASCII whitespace sequences never come through."""
    failures = _fuzz(dfa, list(range(256)), 10_000, seed=7, max_steps=40)
    assert not failures, failures[:5]


def test_liveness_every_reachable_state_reaches_acceptance(dfa):
    states = go.reachable(dfa)
    finish = go.completions(dfa)
    assert len(states) > 50 and dfa.start in states
    dead_ends = [s for s in states if s not in finish]
    assert not dead_ends, dead_ends
    no_insufficient = citation_grammar(go.IDS, allow_insufficient=False)
    finish2 = go.completions(no_insufficient)
    assert all(s in finish2 for s in go.reachable(no_insufficient))
    assert not accepts(no_insufficient, b"INSUFFICIENT_EVIDENCE")


@pytest.mark.parametrize("text", ["Foo [Q-7].", "Foo. [Q-7]", "Foo.[Q-7][A-45]\n- Bar! [Q-12]", "INSUFFICIENT_EVIDENCE",
                                  "See v1.2.3 of the café notes [Q-123]!\n2) second point [A-45][Q-7]"])
def test_accepted(dfa, text):
    assert accepts(dfa, text.encode())
    assert text == answer.INSUFFICIENT or validate_citations(text, go.IDS)["valid"]


@pytest.mark.parametrize("text", ["Foo.", "Foo.\n", "Foo. Bar [Q-7].", "Foo [Q-7]. Bar.", "Foo [Q-1].", "Foo [Q-124].",
                                  "[Q-7]", "24. [A-45]", "Foo [Q-7]. [Q-12] bar", "Foo bar [Q-7].",
                                  "Foo bar [Q-7].", "Foo [Q-7]. ", "Foo [x] [Q-7].", "Foo\r [Q-7].",
                                  "INSUFFICIENT_EVIDENC", ""])
def test_refused(dfa, text):
    assert not accepts(dfa, text.encode())


def test_device_forms_are_contiguous_tensors_of_the_kernels_types(dfa):
    import torch
    table = TokenTable.from_bytes([b"a", b"bc", None], stop_ids=[2])
    tensors = table.to("cpu") + dfa.to("cpu")
    assert [t.dtype for t in tensors] == [torch.int32, torch.uint8, torch.uint8, torch.uint8, torch.int16, torch.uint8]
    assert all(t.is_contiguous() for t in tensors) and tensors[4].shape == (dfa.n_states, dfa.n_classes)
    assert np.array_equal(tensors[4].numpy().view(np.uint16), dfa.trans) and table.to("cpu") is table.to("cpu")


def test_insufficient_constant_is_the_answer_modules():
    assert grammar.INSUFFICIENT.decode() == answer.INSUFFICIENT


def test_walk_and_the_host_rule(dfa):
    table = TokenTable.from_bytes([b"Foo", b" [Q", b"-7]", b"-8]", b"", b"<eos>", b"x", None], stop_ids=[5], never_ids=[6])
    assert table.kind.tolist() == [0, 0, 0, 0, 2, 1, 2, 2] and table.token_bytes(1) == b" [Q"
    assert walk(dfa, dfa.start, b"") == dfa.start and walk(dfa, dfa.start, b"Foo\n") is None
    assert walk(dfa, None, b"a") is None and walk(dfa, dfa.n_states, b"a") is None
    s = walk(dfa, dfa.start, b"Foo [Q")
    assert allowed_tokens_host(dfa, table, s).tolist() == [False, False, True, False, False, False, False, False]
    s = next_state_host(dfa, table, s, 2)
    assert s == walk(dfa, dfa.start, b"Foo [Q-7]") and dfa.accept[s]
    assert allowed_tokens_host(dfa, table, s).tolist() == [True, True, True, True, False, True, False, False]
    assert next_state_host(dfa, table, s, 5) == s and next_state_host(dfa, table, s, -1) == s
    with pytest.raises(ValueError):
        next_state_host(dfa, table, s, 6)
    with pytest.raises(ValueError):
        next_state_host(dfa, table, walk(dfa, dfa.start, b"Foo [Q"), 3)
    assert not allowed_tokens_host(dfa, table, dfa.n_states).any() and not allowed_tokens_host(dfa, table, -1).any()


def test_token_table_of_the_tiny_tokenizer():
    from tiny_checkpoint import build_tokenizer
    tok = build_tokenizer()
    eos = int(tok.eos_token_id)
    table = TokenTable.from_tokenizer(tok, [eos], vocab_size=len(tok) + 5)
    assert table.vocab == len(tok) + 5 and table.kind[eos] == grammar.KIND_STOP
    assert (table.kind[len(tok):] == grammar.KIND_NEVER).all()
    checked = 0
    for i in range(len(tok)):
        if table.kind[i] != grammar.KIND_ORDINARY:
            continue
        raw = table.token_bytes(i)
        assert raw
        try:
            text = raw.decode()
        except UnicodeDecodeError:
            continue
        assert text == tok.decode([i]), (i, raw)
        checked += 1
    assert checked > 256 - 128            # every ASCII byte and the merges
    singles = {table.token_bytes(i) for i in range(len(tok)) if table.kind[i] == grammar.KIND_ORDINARY}
    assert all(bytes([b]) in singles for b in range(256))   # a byte-level vocabulary: decoding never meets an empty set
    ids = tok.encode("Foo. [Q-7]", add_special_tokens=False)
    assert b"".join(table.token_bytes(i) for i in ids) == b"Foo. [Q-7]"
    assert TokenTable.from_tokenizer(tok, []).kind[eos] == grammar.KIND_NEVER


def test_caps():
    with pytest.raises(ValueError, match="states"):
        citation_grammar([f"Q-{10 ** 9 + 7919 * i}" for i in range(200)])
    with pytest.raises(ValueError):
        citation_grammar([])
    with pytest.raises(ValueError, match="evidence id"):
        citation_grammar(["Q-007"])
    with pytest.raises(ValueError):
        ByteDfa(np.zeros(256, np.uint8), np.zeros((4097, 1), np.uint16), np.zeros(4097, np.uint8))
    with pytest.raises(ValueError):
        ByteDfa(np.zeros(256, np.uint8), np.zeros((1, 65), np.uint16), np.zeros(1, np.uint8))
    big = citation_grammar([f"Q-{100 + i}" for i in range(40)] + [f"A-{i}" for i in range(12)])   # a full pack fits
    assert big.n_states <= grammar.MAX_STATES and big.n_classes <= grammar.MAX_CLASSES


def test_grammar_argmax_argument_errors_are_codes(native_lib):
    """The checks of crag_enc_grammar_argmax come before anything is enqueued, so they hold without a GPU: host buffers
    stand in for the device pointers."""
    import ctypes

    from cadence_rag_amd import _native
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = [p, 100, p, p, p, p, p, p, 4, 4, p, p, None, 1, None]
    names = ["logits", "vocab", "tok_offsets", "tok_bytes", "tok_kind", "class_of", "trans", "accept", "n_states",
             "n_classes", "state", "token", "allowed_bits", "n_rows", "stream"]

    def call(**change):
        args = list(good)
        for k, v in change.items():
            args[names.index(k)] = v
        return native_lib.crag_enc_grammar_argmax(*args)

    for name in ("logits", "tok_offsets", "tok_bytes", "tok_kind", "class_of", "trans", "accept", "state", "token"):
        assert call(**{name: None}) == -1 and "NULL" in _native.last_error(), name
    for change, word in (({"n_rows": 0}, "n_rows"), ({"n_rows": _native.CRAG_DECODE_MAX_SEQS + 1}, "n_rows"),
                         ({"n_states": 0}, "n_states"), ({"n_states": grammar.MAX_STATES + 1}, "n_states"),
                         ({"n_classes": 0}, "n_classes"), ({"n_classes": grammar.MAX_CLASSES + 1}, "n_classes"),
                         ({"vocab": 0}, "vocab"), ({"vocab": -5}, "vocab"), ({"vocab": 2 ** 31}, "vocab"),
                         ({"trans": ctypes.c_void_p(p.value + 1)}, "aligned"),
                         ({"state": ctypes.c_void_p(p.value + 2)}, "aligned")):
        assert call(**change) == -1 and word in _native.last_error(), (change, _native.last_error())
    assert (_native.CRAG_GRAMMAR_MAX_STATES, _native.CRAG_GRAMMAR_MAX_CLASSES, _native.CRAG_GRAMMAR_DEAD) == \
        (grammar.MAX_STATES, grammar.MAX_CLASSES, grammar.DEAD)


# ---- answer_question ---------------------------------------------------------------------------------------------------
def _items(n):
    return [{"evidence_id": f"Q-{10 + i}", "call_id": f"call-{i % 2}", "chunk_id": 10 + i, "speaker": "agent",
             "start_ts_ms": 0, "end_ts_ms": 1, "snippet": f"fact number {i}", "why_relevant": "bm25"} for i in range(n)]


@pytest.fixture
def pack(monkeypatch):
    def fake(request, backend=None):
        return {"query_id": "00000000-0000-0000-0000-000000000001", "intent": request.intent, "budget": {},
                "artifacts": [], "quotes": _items(3), "notes": {}}

    monkeypatch.setattr(retrieve, "retrieve_evidence", fake)
    monkeypatch.setattr(settings, "llm_base_url", "native")
    monkeypatch.setattr(settings, "answer_max_repairs", 1)
    yield
    answer.set_llm(None)


class _Plain:
    """A chat model that knows nothing of grammars: an unexpected keyword would be a TypeError."""
    model_id = "stub"

    def __init__(self, too_long_above=None):
        self.calls, self.too_long_above = [], too_long_above

    def generate_text(self, messages, max_new_tokens):
        self.calls.append({})
        return "The fact holds [Q-10]."


class _Grammatical(_Plain):
    supports_grammar = True

    def generate_text(self, messages, max_new_tokens, **kw):
        if self.too_long_above is not None and messages[1]["content"].count("\n[") > self.too_long_above:
            raise ValueError("the prompt does not fit")
        self.calls.append(kw)
        return "The fact holds [Q-10]."


class _WithTable(_Grammatical):
    table = TokenTable.from_bytes([b"a"])

    def token_table(self):
        return self.table


def _same(a: ByteDfa, b: ByteDfa) -> bool:
    return np.array_equal(a.trans, b.trans) and np.array_equal(a.class_of, b.class_of) and \
        np.array_equal(a.accept, b.accept) and a.start == b.start


def test_answer_setting_off_passes_no_grammar(pack, monkeypatch):
    assert settings.answer_constrained is False and type(settings).from_env().answer_constrained is False
    monkeypatch.setenv("ANSWER_CONSTRAINED", "1")
    assert type(settings).from_env().answer_constrained is True
    llm = _Grammatical()
    answer.set_llm(llm)
    out = answer.answer_question(AnswerRequest(query="what holds?"))
    # off, the response is exactly what it was before the setting existed: no grammar, and no note about one
    assert out["status"] == "ok" and llm.calls == [{}] and out["notes"].get("constrained", False) is False
    assert sorted(out["notes"]) == ["dropped_evidence", "evidence_items", "llm_calls", "validator"]


def test_answer_setting_on_passes_the_grammar_of_the_prompts_ids(pack, monkeypatch):
    monkeypatch.setattr(settings, "answer_constrained", True)
    llm = _WithTable()
    answer.set_llm(llm)
    out = answer.answer_question(AnswerRequest(query="what holds?"))
    assert out["status"] == "ok" and out["notes"]["constrained"] is True and "constrained_error" not in out["notes"]
    (kw,) = llm.calls
    assert set(kw) == {"grammar"} and isinstance(kw["grammar"], TokenGrammar) and kw["grammar"].table is llm.table
    assert kw["grammar"].dfa.evidence_ids == ("Q-10", "Q-11", "Q-12")
    assert _same(kw["grammar"].dfa, citation_grammar(["Q-10", "Q-11", "Q-12"]))
    # an item dropped for length: the grammar is rebuilt from what is left in the prompt
    llm = _Grammatical(too_long_above=2)
    answer.set_llm(llm)
    out = answer.answer_question(AnswerRequest(query="what holds?"))
    assert out["notes"]["dropped_evidence"] == 1 and out["notes"]["constrained"] is True
    (kw,) = llm.calls
    assert kw["grammar"].table is None and _same(kw["grammar"].dfa, citation_grammar(["Q-10", "Q-11"]))
    assert not accepts(kw["grammar"].dfa, b"Foo [Q-12].") and accepts(kw["grammar"].dfa, b"Foo [Q-11].")


def test_answer_setting_on_without_support_or_over_http_passes_no_grammar(pack, monkeypatch):
    monkeypatch.setattr(settings, "answer_constrained", True)
    llm = _Plain()
    answer.set_llm(llm)
    out = answer.answer_question(AnswerRequest(query="what holds?"))
    assert out["status"] == "ok" and llm.calls == [{}] and out["notes"]["constrained"] is False
    # an HTTP backend ignores the setting, whatever is registered
    answer.set_llm(_Grammatical())
    monkeypatch.setattr(settings, "llm_base_url", "http://llm.invalid/v1")
    monkeypatch.setattr(answer, "_post_json", lambda url, headers, body, timeout_s: (
        200, '{"choices": [{"message": {"content": "The fact holds [Q-10]."}}], "model": "m"}'))
    out = answer.answer_question(AnswerRequest(query="what holds?"))
    assert out["status"] == "ok" and out["notes"]["constrained"] is False


def test_answer_reports_a_grammar_that_cannot_be_built(pack, monkeypatch):
    monkeypatch.setattr(settings, "answer_constrained", True)

    def fake(request, backend=None):
        items = [dict(_items(1)[0], evidence_id=f"Q-{10 ** 9 + 7919 * i}") for i in range(200)]
        return {"query_id": "00000000-0000-0000-0000-000000000001", "intent": request.intent, "budget": {},
                "artifacts": [], "quotes": items, "notes": {}}

    monkeypatch.setattr(retrieve, "retrieve_evidence", fake)
    llm = _Grammatical()
    answer.set_llm(llm)
    out = answer.answer_question(AnswerRequest(query="what holds?"))
    assert llm.calls[0] == {} and out["notes"]["constrained"] is False and "states" in out["notes"]["constrained_error"]
