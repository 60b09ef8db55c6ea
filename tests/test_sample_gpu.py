"""crag_enc_sample and crag_enc_grammar_advance on the GPU against the host rule (cadence_rag_amd.sampling.sample_host,
grammar.next_state_host).

Exact, no tolerance: greedy rows against crag_enc_lm_head's and crag_enc_grammar_argmax's own tokens, and the three at
the edges of their shared (value, id) merge (the maximum at ids 0 and vocab - 1); with top_p == 1 the
kept count and the lowest kept logit; the same bits when a call is repeated, its rows permuted and padded by others;
every (state, token) step of a citation grammar.
The draw: a case is compared when the fp64 winner is the same under top_p (1 - d) and top_p (1 + d), d = 1e-4 (the fp32
error of a sum of <= 2^18 weights and of expf's argument is about 1e-5), and the two largest keys differ by more than
1e-3 (the fp32 key errors are about 1e-5); then the token must be equal and the kept count lie between the two host
counts.  At least 98 % of the cases must have been compared.
Distribution: 20 000 draws over 16 tokens, chi-square against the softmax below 60 at 15 degrees of freedom (the
1 - 1e-6 quantile is 56.5); the seeds are fixed, so the figure is deterministic."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from cadence_rag_amd.grammar import (KIND_NEVER, ByteDfa, TokenTable, allowed_tokens_host, citation_grammar,
                                     next_state_host)
from cadence_rag_amd.sampling import SamplingParams, sample_host

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIZES = [1, 31, 33, 63, 64, 65, 1023, 1024, 1025, 4097, 151_936]
DELTA, EPS = 1e-4, 1e-3


def _pack(allowed: np.ndarray) -> torch.Tensor:
    """bool [n, V] -> int32 [n, ceil(V / 32)], bit t % 32 of word t / 32."""
    n, v = allowed.shape
    padded = np.zeros((n, (v + 31) // 32 * 32), np.uint8)
    padded[:, :v] = allowed
    words = np.packbits(padded, axis=1, bitorder="little").view(np.uint32)
    return torch.from_numpy(words.view(np.int32).copy()).to(DEV)


def _sample(logits: np.ndarray, params, step, streams, allowed=None):
    """One call: (tokens, kept counts, the bits of cut), lists of n."""
    from cadence_rag_amd.encoder import ops
    n = logits.shape[0]
    lg = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).to(DEV)
    token = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    kept = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    cut = torch.full((n,), 123.0, dtype=torch.float32, device=DEV)
    ops.sample(lg, params, step, streams, token, allowed_bits=None if allowed is None else _pack(allowed), kept=kept,
               cut=cut)
    return token.cpu().tolist(), kept.cpu().tolist(), cut.cpu().numpy().view(np.uint32).tolist()


def _bits(x: float) -> int:
    return int(np.float32(x).view(np.uint32))


def _coarse(rng, n, v):
    """Logits on a grid of 1/4 with sd 3: equal values everywhere, at the maximum and at every threshold too."""
    return (np.round(rng.standard_normal((n, v)) * 12) / 4).astype(np.float32)


# ---- greedy rows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 8])
@pytest.mark.parametrize("v", SIZES)
def test_greedy_rows_equal_lm_head_and_grammar_argmax(gpu, v, rows):
    from cadence_rag_amd.encoder import ops
    rng = np.random.default_rng(v * 10 + rows)
    greedy = SamplingParams(0.0, top_k=min(3, v), top_p=0.5, min_p=0.3)    # the cuts mean nothing to a greedy row
    # lm_head's own logits and token: equal lm rows give equal maxima; an inf weight gives +inf, -inf and NaN logits
    hidden = 64
    hs = torch.from_numpy(rng.standard_normal((rows, hidden)).astype(np.float32)).to(DEV).to(torch.bfloat16)
    lm = rng.standard_normal((v, hidden)).astype(np.float32)
    lm[rng.integers(0, v, max(v // 3, 1))] = lm[rng.integers(0, v)]       # many copies of one row: ties, often at the top
    for k, i in enumerate(rng.integers(0, v, max(v // 50, 2 if v > 4 else 0))):
        lm[i, k % hidden] = np.inf if k % 3 else -np.inf
    if v > 8:
        lm[rng.integers(0, v, 2)] = np.inf                                # +inf and -inf terms in one dot product: NaN
    w = torch.ones(hidden, dtype=torch.bfloat16, device=DEV)
    logits = torch.empty(rows, v, dtype=torch.float32, device=DEV)
    want = torch.empty(rows, dtype=torch.int32, device=DEV)
    ops.lm_head(hs, w, torch.from_numpy(lm).to(DEV).to(torch.bfloat16).contiguous(), logits, want, 1e-6)
    got = torch.empty_like(want)
    ops.sample(logits, greedy, 3, list(range(rows)), got)
    host = logits.cpu().numpy()
    usable = [r for r in range(rows) if (host[r] > -np.inf).any()]           # lm_head alone takes a -inf when all else is NaN
    assert [got[r].item() for r in usable] == [want[r].item() for r in usable]
    assert [got[r].item() for r in range(rows) if r not in usable] == [-1] * (rows - len(usable))

    # planted logits under grammar_argmax's bits: a one-state automaton that lets every byte pass, a fifth of the ids never
    x = _coarse(rng, rows, v)
    x[rng.random((rows, v)) < 0.05] = np.nan
    x[rng.random((rows, v)) < 0.05] = -np.inf
    if rows > 1:
        x[1, rng.integers(0, v, 2)] = np.inf                                 # the lowest id holding +inf
    kind = np.where(rng.random(v) < 0.2, KIND_NEVER, 0).astype(np.uint8)
    table = TokenTable(np.arange(v + 1, dtype=np.int32), np.full(v, 65, np.uint8), kind)
    dfa = ByteDfa(np.zeros(256, np.uint8), np.zeros((1, 1), np.uint16), np.ones(1, np.uint8))
    lg = torch.from_numpy(x).to(DEV)
    state = torch.zeros(rows, dtype=torch.int32, device=DEV)
    bits = torch.empty(rows, (v + 31) // 32, dtype=torch.int32, device=DEV)
    ops.grammar_argmax(lg, *table.to(DEV), *dfa.to(DEV), state, want, allowed_bits=bits)
    kept = torch.empty(rows, dtype=torch.int32, device=DEV)
    cut = torch.empty(rows, dtype=torch.float32, device=DEV)
    ops.sample(lg, greedy, 0, [0] * rows, got, allowed_bits=bits, kept=kept, cut=cut)
    allowed = kind == 0
    for r in range(rows):
        ref = sample_host(x[r], greedy, 0, 0, allowed=allowed)
        assert (got[r].item(), kept[r].item()) == (ref.token, ref.kept), (r, ref)
        assert ref.token < 0 or _bits(cut[r].item()) == _bits(ref.cut)
        if ref.token >= 0 or not (allowed & (x[r] == -np.inf)).any():        # grammar_argmax takes a -inf when nothing else is left
            assert want[r].item() == ref.token, (r, ref)
    # nothing allowed: -1 and a kept count of 0
    token, kept, _ = _sample(x, greedy, 0, [0] * rows, allowed=np.zeros((rows, v), bool))
    assert token == [-1] * rows and kept == [0] * rows
    token, kept, _ = _sample(x, SamplingParams(1.0), 0, [0] * rows, allowed=np.zeros((rows, v), bool))
    assert token == [-1] * rows and kept == [0] * rows


@pytest.mark.parametrize("v", [63, 64, 65, 1024, 1025])
def test_the_maximum_at_the_first_and_the_last_id_goes_to_the_lower_one(gpu, v):
    """The (value, id) merge at its edges: below and above one wave, below and above one pass of the 1024 threads.  The
    maximum sits at ids 0 and v - 1 alone -- thread 0 and the last thread that holds an id -- and lm_head's token,
    grammar_argmax in a state that allows everything and sample at T = 0 all name id 0; with id 0 banned, or its logit
    NaN, they all name v - 1."""
    from cadence_rag_amd.encoder import ops
    rng = np.random.default_rng(v)
    rows, hidden = 2, 64
    x = rng.standard_normal((rows, hidden)).astype(np.float32)
    x[:, :2] = 1.0
    lm = (rng.standard_normal((v, hidden)) * 0.1).astype(np.float32)
    lm[0] = lm[v - 1] = np.sign(x[0]) * (np.sign(x[0]) == np.sign(x[1])) * 4.0    # a large dot product with both rows
    hs = torch.from_numpy(x).to(DEV).to(torch.bfloat16)
    w = torch.ones(hidden, dtype=torch.bfloat16, device=DEV)
    lmw = torch.from_numpy(lm).to(DEV).to(torch.bfloat16).contiguous()
    logits = torch.empty(rows, v, dtype=torch.float32, device=DEV)
    token = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    ops.lm_head(hs, w, lmw, logits, token, 1e-6)
    host = logits.cpu().numpy()
    top = host.max(1)
    assert [np.flatnonzero(host[r] == top[r]).tolist() for r in range(rows)] == [[0, v - 1]] * rows
    assert token.tolist() == [0] * rows
    greedy = SamplingParams(0.0)
    kind = np.zeros(v, np.uint8)
    dfa = ByteDfa(np.zeros(256, np.uint8), np.zeros((1, 1), np.uint16), np.ones(1, np.uint8)).to(DEV)

    def grammar_token(lg, kind, with_bits):
        table = TokenTable(np.arange(v + 1, dtype=np.int32), np.full(v, 65, np.uint8), kind).to(DEV)
        state = torch.zeros(rows, dtype=torch.int32, device=DEV)
        out = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
        bits = torch.empty(rows, (v + 31) // 32, dtype=torch.int32, device=DEV) if with_bits else None
        ops.grammar_argmax(lg, *table, *dfa, state, out, allowed_bits=bits)
        return out.tolist(), bits

    def sample_token(lg, bits):
        out = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
        ops.sample(lg, greedy, 0, [0] * rows, out, allowed_bits=bits)
        return out.tolist()

    for with_bits in (False, True):
        got, bits = grammar_token(logits, kind, with_bits)
        assert got == [0] * rows and sample_token(logits, bits) == [0] * rows
    # id 0 banned
    ops.lm_head(hs, w, lmw, logits, token, 1e-6, banned=torch.zeros(1, dtype=torch.int32, device=DEV))
    assert token.tolist() == [v - 1] * rows
    banned_kind = kind.copy()
    banned_kind[0] = KIND_NEVER
    for with_bits in (False, True):
        got, bits = grammar_token(logits, banned_kind, with_bits)
        assert got == [v - 1] * rows
    assert sample_token(logits, bits) == [v - 1] * rows
    # id 0 NaN: an inf and a -inf weight meet in its dot product
    lm[0, :2] = [np.inf, -np.inf]
    ops.lm_head(hs, w, torch.from_numpy(lm).to(DEV).to(torch.bfloat16).contiguous(), logits, token, 1e-6)
    assert torch.isnan(logits[:, 0]).all() and token.tolist() == [v - 1] * rows
    for with_bits in (False, True):
        got, bits = grammar_token(logits, kind, with_bits)
        assert got == [v - 1] * rows and sample_token(logits, bits) == [v - 1] * rows


# ---- the cuts, exactly ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 8])
@pytest.mark.parametrize("v", SIZES)
def test_kept_and_cut_equal_the_host_without_top_p(gpu, v, rows):
    rng = np.random.default_rng(v * 7 + rows)
    combos = [SamplingParams(0.7, top_k=min(k, v), min_p=mp, seed=5) for k in (1, 2, 7, v) for mp in (0.0, 0.05, 1.0)]
    x = _coarse(rng, 8, v)                               # ties at every threshold: the grid has about 100 values
    allowed = rng.random((8, v)) < 0.8                   # v is no multiple of 32 for most sizes: a partial last word
    allowed[:, rng.integers(0, v)] = True
    for lo in range(0, 16 if rows == 8 else 12, rows):
        params = [combos[(lo + r) % len(combos)] for r in range(rows)]
        for with_bits in (False, True):
            al = allowed[:rows] if with_bits else None
            token, kept, cut = _sample(x[:rows], params, lo, list(range(rows)), allowed=al)
            for r in range(rows):
                ref = sample_host(x[r], params[r], lo, r, allowed=None if al is None else al[r])
                assert (kept[r], cut[r]) == (ref.kept, _bits(ref.cut)), (v, r, params[r], kept[r], ref)
                assert 0 <= token[r] < v and (al is None or al[r, token[r]]) and x[r, token[r]] >= ref.cut
                if ref.gap > EPS:
                    assert token[r] == ref.token, (v, r, params[r], token[r], ref)


def test_minus_zero_and_plus_zero_are_one_value(gpu):
    x = np.array([[-1.0, -0.0, 0.0, -2.0, 0.0, -0.0]], np.float32)
    for params in (SamplingParams(1.0, top_k=1), SamplingParams(1.0, min_p=1.0), SamplingParams(0.0)):
        token, kept, cut = _sample(x, params, 0, [0])
        assert kept == [4] and np.uint32(cut[0]).view(np.float32) == 0.0 and token[0] in (1, 2, 4, 5)
    assert _sample(x, SamplingParams(0.0), 0, [0])[0] == [1]


# ---- determinism and independence ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [1025, 151_936])
def test_a_rows_outputs_do_not_depend_on_the_call(gpu, v):
    rng = np.random.default_rng(v)
    x = (rng.standard_normal((8, v)) * 3).astype(np.float32)
    allowed = rng.random((8, v)) < 0.7
    params = [SamplingParams(1.0, seed=3), SamplingParams(0.7, top_k=50, seed=3), SamplingParams(0.7, top_p=0.9, seed=3),
              SamplingParams(1.0, top_p=0.9, min_p=0.05, seed=3), SamplingParams(0.0, seed=3),
              SamplingParams(0.3, top_k=7, top_p=0.5, seed=3), SamplingParams(2.0, top_p=0.99, seed=3),
              SamplingParams(0.7, min_p=0.01, seed=3)]
    streams = [4, 0, 9, 2, 7, 1, 3, 8]
    first = _sample(x, params, 11, streams, allowed=allowed)
    assert _sample(x, params, 11, streams, allowed=allowed) == first
    for order in ([7, 6, 5, 4, 3, 2, 1, 0], [2], [5, 5, 0], [3, 1, 4, 1, 5, 2, 6, 5]):
        again = _sample(x[order], [params[i] for i in order], 11, [streams[i] for i in order], allowed=allowed[order])
        for out, ref in zip(again, first):
            assert out == [ref[i] for i in order], order
    other = _sample(x, params, 12, streams, allowed=allowed)
    assert other[1:] == first[1:] and other[0] != first[0]      # another step: other draws, the same cuts


# ---- the draw ---------------------------------------------------------------------------------------------------------------
def _draw_params(v):
    return [SamplingParams(1.0, seed=17), SamplingParams(0.7, top_k=min(50, v), seed=17),
            SamplingParams(0.7, top_p=0.9, seed=17), SamplingParams(1.0, top_p=0.9, min_p=0.05, seed=17),
            SamplingParams(0.5, top_k=min(7, v), top_p=0.8, seed=17), SamplingParams(1.5, top_p=0.95, seed=17),
            SamplingParams(0.7, min_p=0.02, seed=17), SamplingParams(0.2, top_p=0.5, seed=17)]


@pytest.mark.parametrize("v", SIZES)
def test_the_draw_equals_the_host_where_the_host_is_sure(gpu, v):
    """Calls of 1 row and of 8 rows, with and without allowed_bits; 64 cases at the real vocabulary, 120 elsewhere."""
    rng = np.random.default_rng(v * 3)
    compared = total = 0
    for rows, calls in ((1, 8 if v > 100_000 else 24), (8, 7 if v > 100_000 else 12)):
        for call in range(calls):
            x = (rng.standard_normal((rows, v)) * rng.choice([2.0, 3.0, 4.0])).astype(np.float32)
            al = (rng.random((rows, v)) < 0.75) if call % 2 else None
            if al is not None:
                al[:, rng.integers(0, v)] = True
            params = [_draw_params(v)[(call + r) % 8] for r in range(rows)]
            streams = [int(s) for s in rng.integers(0, 1000, rows)]
            token, kept, _ = _sample(x, params, call, streams, allowed=al)
            for r in range(rows):
                ref = sample_host(x[r], params[r], call, streams[r], allowed=None if al is None else al[r], delta=DELTA)
                total += 1
                if not (ref.stable and ref.gap > EPS):
                    continue
                compared += 1
                assert token[r] == ref.token, (v, rows, call, r, params[r], token[r], ref)
                assert ref.kept_lo <= kept[r] <= ref.kept_hi, (v, rows, call, r, params[r], kept[r], ref)
    print(f"V {v}: {compared} of {total} cases compared")
    assert compared >= 0.98 * total, (compared, total)


# ---- the distribution -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_draws_follow_the_softmax(gpu, temperature):
    from cadence_rag_amd.encoder import ops
    p = np.geomspace(0.3, 0.002, 16)
    p /= p.sum()
    logits = torch.from_numpy(np.tile(np.log(p).astype(np.float32), (8, 1))).to(DEV)
    params = SamplingParams(temperature, seed=20261019)
    out = torch.empty(2500, 8, dtype=torch.int32, device=DEV)
    for step in range(2500):
        ops.sample(logits, params, step, list(range(8)), out[step])
    counts = np.bincount(out.cpu().numpy().ravel(), minlength=16)
    want = p ** (1.0 / temperature)
    want *= 20_000 / want.sum()
    chi2 = float(((counts - want) ** 2 / want).sum())
    print(f"T {temperature}: chi2 {chi2:.2f}, counts {counts.tolist()}")
    assert counts.sum() == 20_000 and counts.size == 16
    assert chi2 < 60.0, chi2


# ---- grammar_advance --------------------------------------------------------------------------------------------------------
def test_grammar_advance_equals_the_host_rule_for_every_state_and_token(gpu):
    from cadence_rag_amd.encoder import ops
    ids = [f"Q-{n}" for n in (7, 12, 13, 123, 124, 130, 2000, 45)] + [f"A-{n}" for n in (1, 45, 46, 900)]
    dfa = citation_grammar(ids)
    tokens = [b"Foo", b" bar", b".", b". ", b" [", b"[Q", b"[A", b"-1", b"-", b"2", b"3", b"23]", b"]", b"].", b"]\n", b"\n",
              b"[Q-7]", b"[A-45] ", b"[Q-8]", b"INSUFFICIENT", b"_EVIDENCE", b"!?", b" ", b"\t", b"x", b"0", b"45", b"00]",
              "é".encode(), b"\xc2", b"\xa0", b"\r", None, b"<eos>", b"<stop>", b"never"]
    stop, never = [33, 34], [35]
    table = TokenTable.from_bytes(tokens, stop_ids=stop, never_ids=never)
    v = table.vocab
    pairs = [(s, t) for s in range(dfa.n_states) for t in list(range(v)) + [-1, v, v + 1000]]
    pairs += [(-1, 0), (dfa.n_states, 0), (dfa.n_states + 7, 2)]          # a state outside the table stays
    allowed = {s: allowed_tokens_host(dfa, table, s) for s in range(dfa.n_states)}
    want = []
    for s, t in pairs:
        ok = 0 <= s < dfa.n_states and (t < 0 or (t < v and allowed[s][t]))
        want.append(next_state_host(dfa, table, s, t) if ok and t < v else s)
    moved = sum(w != s for w, (s, _) in zip(want, pairs))
    assert moved > len(pairs) // 10 and dfa.n_states > 100
    tabs = table.to(DEV) + dfa.to(DEV)[:2]
    got = []
    states = torch.tensor([s for s, _ in pairs], dtype=torch.int32)
    toks = torch.tensor([t for _, t in pairs], dtype=torch.int32)
    for lo in range(0, len(pairs), 8):
        st = states[lo:lo + 8].to(DEV)
        tk = toks[lo:lo + 8].to(DEV)
        ops.grammar_advance(*tabs, st, tk)
        got.append(st)
        assert torch.equal(tk.cpu(), toks[lo:lo + 8])
    got = torch.cat(got).cpu().tolist()
    wrong = [(pairs[i], got[i], want[i]) for i in range(len(pairs)) if got[i] != want[i]]
    assert not wrong, wrong[:8]
    one = torch.tensor([dfa.start], dtype=torch.int32, device=DEV)       # a single row
    ops.grammar_advance(*tabs, one, torch.tensor([0], dtype=torch.int32, device=DEV))
    assert one.item() == next_state_host(dfa, table, dfa.start, 0)
