"""crag_enc_grammar_argmax on the GPU against the host rule (cadence_rag_amd.grammar): allowed flags bit for bit, the
lowest-id argmax over the allowed tokens and the next state, in every reachable state of a citation grammar; the call
without allowed_bits; rows with nothing allowed; the transition table in LDS and through the cache, at both sides of the switch; argument
errors.  Then Qwen3Generator.generate(grammar=...) on the tiny checkpoint against a host-driven loop over the same
logits, and /answer through the native backend with ANSWER_CONSTRAINED."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import grammar_oracle as go
from cadence_rag_amd import grammar
from cadence_rag_amd.grammar import (ByteDfa, TokenGrammar, TokenTable, allowed_tokens_host, argmax_host,
                                     citation_grammar, next_state_host, walk)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MAX_ROWS = 8
V = go.VOCAB


@pytest.fixture(scope="module")
def dfa():
    return citation_grammar(go.IDS)


@pytest.fixture(scope="module")
def vocab():
    return go.synthetic_vocab()


@pytest.fixture(scope="module")
def logits():
    """[8, 3001] fp32: few distinct values, so equal maxima among the allowed tokens (and an equal value at a lower id
    that is not allowed) occur in most states; NaNs at 5 % of the ids; per row the top value planted at six ids."""
    rng = np.random.default_rng(3)
    x = rng.integers(0, 40, (MAX_ROWS, V)).astype(np.float32) * 0.25
    for r in range(MAX_ROWS):
        x[r, rng.choice(V, 6, replace=False)] = 10.0
    x[rng.random((MAX_ROWS, V)) < 0.05] = np.nan
    return x


@pytest.fixture(scope="module")
def host(dfa, vocab):
    """state -> bool[V] of the host rule, for every reachable state; computed once."""
    table, _ = vocab
    return {s: allowed_tokens_host(dfa, table, s) for s in go.reachable(dfa)}


def _run(dfa: ByteDfa, table: TokenTable, logits_np: np.ndarray, states, bits: bool):
    """One call of ops.grammar_argmax: (tokens, new states, allowed bool [n, V] or None, the words beyond V)."""
    from cadence_rag_amd.encoder import ops
    n = len(states)
    lg = torch.from_numpy(np.ascontiguousarray(logits_np[:n])).to(DEV)
    st = torch.tensor(list(states), dtype=torch.int32, device=DEV)
    tok = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    words = (V + 31) // 32
    ab = torch.full((n, words), -1, dtype=torch.int32, device=DEV) if bits else None
    ops.grammar_argmax(lg, *table.to(DEV), *dfa.to(DEV), st, tok, allowed_bits=ab)
    flags = tail = None
    if bits:
        raw = np.unpackbits(ab.cpu().numpy().view(np.uint8).reshape(n, -1), axis=1, bitorder="little")
        flags, tail = raw[:, :V].astype(bool), raw[:, V:]
    return tok.cpu().tolist(), st.cpu().tolist(), flags, tail


def _expect(dfa, table, allowed, logits_row, state):
    token = argmax_host(logits_row, allowed)
    return token, next_state_host(dfa, table, state, token)


@pytest.mark.parametrize("rows", [1, MAX_ROWS])
def test_every_reachable_state_against_the_host_rule(gpu, dfa, vocab, logits, host, rows):
    table, special = vocab
    states = list(host)
    assert len(states) > 100
    ties = shadowed = 0
    for lo in range(0, len(states), rows):
        call = states[lo:lo + rows]
        lg = logits[lo % MAX_ROWS:lo % MAX_ROWS + 1] if rows == 1 else logits
        tok, new, flags, tail = _run(dfa, table, lg, call, bits=True)
        assert not tail.any()
        for r, s in enumerate(call):
            assert np.array_equal(flags[r], host[s]), (s, np.nonzero(flags[r] != host[s])[0][:8])
            want_tok, want_state = _expect(dfa, table, host[s], lg[r], s)
            assert (tok[r], new[r]) == (want_tok, want_state), (s, tok[r], want_tok, new[r], want_state)
            if want_tok >= 0:
                top = lg[r, want_tok]
                ties += int((host[s] & (lg[r] == top)).sum() > 1)
                shadowed += int((~host[s][:want_tok] & (lg[r, :want_tok] == top)).any())
    # the cases the logits were shaped for did occur: equal maxima among the allowed, and an equal value at a lower,
    # refused id
    assert ties > len(states) // 4 and shadowed > len(states) // 4, (ties, shadowed)
    for s in states:                       # the fixed kinds, whatever the state
        assert not host[s][special["empty"]].any() and not host[s][special["never"]].any()
        assert host[s][special["stop"]].all() == bool(dfa.accept[s]) == host[s][special["stop"]].any()


def test_the_call_without_allowed_bits_gives_the_same(gpu, dfa, vocab, logits, host):
    table, _ = vocab
    states = list(host)
    for lo in (0, 8, len(states) - MAX_ROWS):
        call = states[lo:lo + MAX_ROWS]
        with_bits = _run(dfa, table, logits, call, bits=True)[:2]
        without = _run(dfa, table, logits, call, bits=False)[:2]
        assert with_bits == without
        assert without[0] == [argmax_host(logits[r], host[s]) for r, s in enumerate(call)]
    one = _run(dfa, table, logits[5:6], [states[17]], bits=False)
    assert one[0] == [argmax_host(logits[5], host[states[17]])]


def test_rows_with_nothing_allowed(gpu, dfa, vocab, logits, host):
    table, special = vocab
    # a one-state automaton whose every transition is dead: nothing is allowed, the state stays
    dead = ByteDfa(np.zeros(256, np.uint8), np.full((1, 1), grammar.DEAD, np.uint16), np.zeros(1, np.uint8))
    tok, new, flags, _ = _run(dead, table, logits, [0] * MAX_ROWS, bits=True)
    assert tok == [-1] * MAX_ROWS and new == [0] * MAX_ROWS and not flags.any()
    # ... accepting, its stop tokens are allowed and nothing else
    dead_ok = ByteDfa(np.zeros(256, np.uint8), np.full((1, 1), grammar.DEAD, np.uint16), np.ones(1, np.uint8))
    tok, new, flags, _ = _run(dead_ok, table, logits, [0, 0], bits=True)
    only_stops = np.zeros(V, bool)
    only_stops[special["stop"]] = True
    assert np.array_equal(flags[0], only_stops) and new == [0, 0]
    assert tok == [argmax_host(logits[r], only_stops) for r in range(2)] and set(tok) <= set(special["stop"])
    # the citation grammar with such a state appended, rows in it and rows outside the table among ordinary rows
    n = dfa.n_states
    trans = np.vstack([dfa.trans, np.full((1, dfa.n_classes), grammar.DEAD, np.uint16)])
    mixed = ByteDfa(dfa.class_of, trans, np.append(dfa.accept, 0), dfa.start)
    good = [s for s in host if host[s].any()][:4]
    call = [good[0], n, good[1], n + 1, good[2], -1, n, good[3]]
    for bits in (True, False):
        tok, new, flags, _ = _run(mixed, table, logits, call, bits=bits)
        for r, s in enumerate(call):
            if s in good:
                assert (tok[r], new[r]) == _expect(dfa, table, host[s], logits[r], s)
                assert flags is None or np.array_equal(flags[r], host[s])
            else:
                assert tok[r] == -1 and new[r] == s and (flags is None or not flags[r].any())


LDS_ENTRIES = 24576     # crag_grammar.hip keeps a transition table of up to this many entries in LDS


@pytest.mark.parametrize("big_n", [599, 600, 4096], ids=["largest_in_lds", "first_through_cache", "cap"])
def test_the_table_in_lds_and_through_the_cache(gpu, dfa, vocab, logits, host, big_n):
    """Both sides of the switch between the two instantiations, and the cap: at 41 classes 599 states (24 559 entries,
    48 KiB of LDS) are the largest table staged in LDS, 600 (24 600) the first read through the cache, 4096 the most
    the entry takes.  The citation grammar's states are scattered over 0..big_n - 1 by a seeded permutation, the rest
    is unreachable padding.  Same flags, tokens and states as the host rule."""
    table, _ = vocab
    assert dfa.n_classes == 41 and 599 * 41 <= LDS_ENTRIES < 600 * 41 and big_n >= dfa.n_states
    perm = np.random.default_rng(9).permutation(big_n)[:dfa.n_states]
    trans = np.full((big_n, dfa.n_classes), grammar.DEAD, np.uint16)
    alive = dfa.trans < dfa.n_states
    trans[perm] = np.where(alive, perm[np.minimum(dfa.trans, dfa.n_states - 1)], grammar.DEAD).astype(np.uint16)
    accept = np.zeros(big_n, np.uint8)
    accept[perm] = dfa.accept
    big = ByteDfa(dfa.class_of, trans, accept, int(perm[dfa.start]))
    assert int(perm.max()) > big_n * 3 // 4
    states = list(host)
    for lo in (0, 40, len(states) - MAX_ROWS):
        call = states[lo:lo + MAX_ROWS]
        for bits in (True, False):
            tok, new, flags, _ = _run(big, table, logits, [int(perm[s]) for s in call], bits=bits)
            for r, s in enumerate(call):
                want_tok, want_state = _expect(dfa, table, host[s], logits[r], s)
                assert (tok[r], new[r]) == (want_tok, int(perm[want_state]))
                assert flags is None or np.array_equal(flags[r], host[s])


def test_argument_errors(gpu, dfa, vocab):
    from cadence_rag_amd import _native
    from cadence_rag_amd.encoder import ops
    table, _ = vocab
    lib = _native.load()
    off, data, kind = table.to(DEV)
    cls, trans, accept = dfa.to(DEV)
    lg = torch.full((MAX_ROWS + 1, V), 1.0, dtype=torch.float32, device=DEV)
    st = torch.zeros(MAX_ROWS + 1, dtype=torch.int32, device=DEV)
    tok = torch.full((MAX_ROWS + 1,), -7, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    good = dict(logits=p(lg), vocab=V, off=p(off), data=p(data), kind=p(kind), cls=p(cls), trans=p(trans), accept=p(accept),
                n_states=dfa.n_states, n_classes=dfa.n_classes, state=p(st), token=p(tok), bits=None, n_rows=2)

    def call(**change):
        a = dict(good, **change)
        return lib.crag_enc_grammar_argmax(a["logits"], a["vocab"], a["off"], a["data"], a["kind"], a["cls"], a["trans"],
                                           a["accept"], a["n_states"], a["n_classes"], a["state"], a["token"], a["bits"],
                                           a["n_rows"], None)

    for name in ("logits", "off", "data", "kind", "cls", "trans", "accept", "state", "token"):
        assert call(**{name: None}) == -1 and "NULL" in _native.last_error(), name
    for change, word in (({"n_rows": 0}, "n_rows"), ({"n_rows": MAX_ROWS + 1}, "n_rows"), ({"n_states": 0}, "n_states"),
                         ({"n_states": 4097}, "n_states"), ({"n_classes": 0}, "n_classes"), ({"n_classes": 65}, "n_classes"),
                         ({"vocab": 0}, "vocab"), ({"vocab": 2 ** 31}, "vocab"),
                         ({"trans": ctypes.c_void_p(trans.data_ptr() + 1)}, "aligned")):
        assert call(**change) == -1 and word in _native.last_error(), (change, _native.last_error())
    with pytest.raises(_native.NativeLibraryError, match="n_rows"):
        ops.grammar_argmax(lg, off, data, kind, cls, trans, accept, st, tok)
    torch.cuda.synchronize()
    assert bool((tok == -7).all()) and bool((st == 0).all())          # nothing was enqueued
    assert call() == 0
    torch.cuda.synchronize()
    assert tok[:2].cpu().tolist() != [-7, -7]


# ---- the generator -----------------------------------------------------------------------------------------------------
NEW = 48
TEXTS = ["the customer called about a failed deployment of the api gateway and we saw ECONNRESET errors between the "
         "gateway and the billing service after the upgrade",
         "ticket ABC-123 tracks the rollback to version v1.2.3 and the follow up call next week, the agent confirmed the "
         "refund and scheduled a call back for tuesday morning, latency went from forty milliseconds to nine hundred",
         "please send the transcript and the action items to the account team, the speaker asked whether the embedding "
         "backfill had finished for all chunks"]
PRIMED = 40      # tokens of every prompt its slot already holds in the reuse_prefix runs


@pytest.fixture(scope="module")
def generator(tmp_path_factory):
    """The tiny checkpoint (2 random layers, byte-level BPE of 384 ids), its embedding table as the head."""
    from tiny_checkpoint import build_checkpoint
    from cadence_rag_amd.encoder.generate import Qwen3Generator
    from cadence_rag_amd.encoder.qwen3 import Qwen3Encoder
    root = tmp_path_factory.mktemp("grammar_tiny")
    build_checkpoint(root)
    enc = Qwen3Encoder.from_pretrained(str(root), DEV, max_length=2048)
    return Qwen3Generator(enc, enc.embed, enc.tokenizer, max_context=2048, max_seqs=4, model_id="tiny")


def _host_generate(gen, prompts, n_new, g: TokenGrammar, reuse: bool):
    """generate(grammar=g) with every selection made on the host from the logits the generator returns."""
    from cadence_rag_amd.encoder.generate import plan_reuse
    dfa, table = g.dfa, g.table
    if reuse:
        keeps = [plan_reuse(gen.resident(b), p) for b, p in enumerate(prompts)]
        assert all(keeps)
        for b, keep in enumerate(keeps):
            gen.truncate(b, keep)
        logits = gen.extend([list(p[keep:]) for p, keep in zip(prompts, keeps)])
    else:
        logits = gen.prefill(prompts)
    states = [dfa.start] * len(prompts)
    trail = [[dfa.start] for _ in prompts]

    def select(rows, lg):
        lg = lg.cpu().numpy()
        picked = []
        for j, b in enumerate(rows):
            t = argmax_host(lg[j], allowed_tokens_host(dfa, table, states[b]))
            states[b] = next_state_host(dfa, table, states[b], t)
            trail[b].append(states[b])
            picked.append(t)
        return picked

    out = [[] for _ in prompts]
    accepted = [False] * len(prompts)
    live = list(range(len(prompts)))
    nxt = select(live, logits)
    while live:
        feed, keep = [], []
        for b, t in zip(live, nxt):
            if t >= 0 and table.kind[t] == grammar.KIND_STOP:
                accepted[b] = True
                continue
            if t < 0:
                continue
            out[b].append(t)
            if len(out[b]) < n_new:
                keep.append(b)
                feed.append(t)
        live = keep
        if not live:
            break
        gen.live = list(live)
        _, logits = gen.step(feed)
        nxt = select(live, logits)
    gen.live = []
    return out, accepted


@pytest.mark.parametrize("reuse", [False, True], ids=["prefill", "reuse_prefix"])
def test_generate_under_a_grammar_equals_the_host_driven_loop(gpu, generator, reuse):
    from cadence_rag_amd.answer import validate_citations
    gen = generator
    tok = gen.tokenizer
    ids = ["Q-12", "A-45"]
    g = TokenGrammar(citation_grammar(ids), gen.token_table())
    assert g.table.vocab == gen.cfg.vocab_size and g.table is gen.token_table()
    prompts = [tok.encode(t, add_special_tokens=False) for t in TEXTS]
    assert min(len(p) for p in prompts) > PRIMED + 1 and len({len(p) for p in prompts}) == 3

    def prime():
        if reuse:
            gen.prefill([p[:PRIMED] for p in prompts])

    prime()
    want, want_accepted = _host_generate(gen, prompts, NEW, g, reuse)
    prime()
    got = gen.generate(prompts, NEW, gen.stop_ids(), reuse_prefix=reuse, grammar=g)
    if reuse:
        assert gen.last_reuse["reused"] == [PRIMED] * 3
    assert got == want and gen.last_grammar == {"accepted": want_accepted} and gen.live == []
    for b, out in enumerate(got):
        assert out and all(g.table.kind[t] == grammar.KIND_ORDINARY for t in out)
        state = g.dfa.start
        for t in out:                                      # every prefix is alive in the host automaton
            state = walk(g.dfa, state, g.table.token_bytes(t))
            assert state is not None
        text = b"".join(g.table.token_bytes(t) for t in out).decode("utf-8", "replace")
        assert "[" not in text or all(i in ids for i in _cited(text))
        print(f"{'reuse' if reuse else 'prefill'} prompt {b}: accepted {want_accepted[b]}, {len(out)} tokens, {text!r}")
        if want_accepted[b]:
            assert bool(g.dfa.accept[state])
            assert text == "INSUFFICIENT_EVIDENCE" or validate_citations(text, ids)["valid"], text
        else:
            assert len(out) == NEW
    # a budget that ends a sequence in the middle of its answer is not an acceptance
    if not reuse:
        assert gen.generate(prompts, 3, gen.stop_ids(), grammar=g) == [w[:3] for w in want]
        assert gen.last_grammar["accepted"] == [a and len(w) < 3 for a, w in zip(want_accepted, want)]


def _cited(text):
    import re
    return [f"{a}-{int(b)}" for a, b in re.findall(r"\[(Q|A)-(\d+)\]", text)]


def test_generate_without_a_grammar_is_the_greedy_path(gpu, generator):
    gen = generator
    prompts = [gen.tokenizer.encode(t, add_special_tokens=False) for t in TEXTS[:2]]
    gen.prefill(prompts)
    by_hand = [[int(t)] for t in gen.last_tokens.tolist()]
    while len(by_hand[0]) < 12:
        token, _ = gen.step([s[-1] for s in by_hand])
        for s, t in zip(by_hand, token.tolist()):
            s.append(int(t))
    assert gen.generate(prompts, 12) == by_hand and gen.last_grammar is None
    assert gen.generate(prompts, 12, grammar=None) == by_hand
    g = TokenGrammar(citation_grammar(["Q-12"]), TokenTable.from_bytes([b"a"] * 7))
    with pytest.raises(ValueError, match="token table"):
        gen.generate(prompts, 4, grammar=g)


def test_answer_constrained_through_the_native_backend(gpu, generator, monkeypatch):
    """A random model writes garbage: unconstrained it fails the citation check with every repair; constrained it can
    cite nothing outside the pack (and whatever it finishes by itself is valid)."""
    from cadence_rag_amd import answer, retrieve
    from cadence_rag_amd.config import settings
    items = [{"evidence_id": f"Q-{10 + i}", "call_id": f"call-{i % 2}", "chunk_id": 10 + i, "speaker": "agent",
              "start_ts_ms": 0, "end_ts_ms": 1, "snippet": f"fact number {i}", "why_relevant": "bm25"} for i in range(3)]

    def fake(request, backend=None):
        return {"query_id": "00000000-0000-0000-0000-000000000001", "intent": request.intent, "budget": {},
                "artifacts": [], "quotes": [dict(i) for i in items], "notes": {}}

    monkeypatch.setattr(retrieve, "retrieve_evidence", fake)
    monkeypatch.setattr(settings, "llm_base_url", "native")
    monkeypatch.setattr(settings, "llm_max_new_tokens", 24)
    monkeypatch.setattr(settings, "answer_max_repairs", 1)
    answer.set_llm(generator)
    try:
        monkeypatch.setattr(settings, "answer_constrained", False)
        plain = answer.answer_question(answer.AnswerRequest(query="what holds?"))
        monkeypatch.setattr(settings, "answer_constrained", True)
        out = answer.answer_question(answer.AnswerRequest(query="what holds?"))
    finally:
        answer.set_llm(None)
    print(f"unconstrained: {plain['status']} {plain['notes']['validator']}\nconstrained: {out['status']} "
          f"{out['notes']['validator']} accepted {generator.last_grammar}")
    assert "constrained" not in plain["notes"] and plain["status"] == "citation_check_failed"
    assert out["notes"]["constrained"] is True and "constrained_error" not in out["notes"]
    assert out["status"] in ("ok", "insufficient_evidence", "citation_check_failed")
    report = out["notes"]["validator"]
    assert report is None or report["unknown_ids"] == []
    if generator.last_grammar["accepted"][0] and out["status"] != "insufficient_evidence":
        assert out["status"] == "ok" and answer.validate_citations(out["answer"], [i["evidence_id"] for i in items])["valid"]
