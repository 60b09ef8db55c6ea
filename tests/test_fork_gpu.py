"""crag_enc_decode_attention_shared and Qwen3Generator.generate_samples on the GPU.

The kernel: bit equality of the outputs and of the appended rows with crag_enc_decode_attention on private copies of
the logical rows, over shared lengths around the 16-key pass and the 128-key split, ragged private suffixes, groups of
2, 3 and 8, several groups in one call, a parent outside the call, other orders and slots; every cache row that must not
be read is NaN.  One case against the fp32 formula, the degenerate arguments, the refusals.
The generator, on the tiny checkpoint: generate_samples token for token against a hand loop over tensor copies of the
prompt's rows and the plain step; under the grammar; with the parent stopping early; n = 1; what the slots hold
afterwards; the fork rules; and that a plain generate never reaches the new entry."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import pytest
import torch

import decode_probes as dp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF = torch.bfloat16
MAX_LEN = 512
N_SLOTS = 10
HEADS = pytest.mark.parametrize("heads", [(8, 2), (4, 2)], ids=["group4", "group2"])
SHARED = [0, 1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 300]
PRIVATE = [0, 1, 127, 128]


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- kernel cases -----------------------------------------------------------------------------------------------
@dataclass
class Seq:
    """One logical sequence.  `key` seeds its data (its new row, and the rows it owns), whatever slot and place in the
    call it gets.  parent: the key of the Seq whose first `shared` rows it reads (None: not forked); it owns `private`
    rows behind them.  in_call False: a finished parent, whose rows stay."""
    key: int
    slot: int
    private: int
    parent: Optional[int] = None
    shared: int = 0
    in_call: bool = True


def _rows(key: int, what: int, n: int, hkv: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(1000 * key + what)
    return torch.randn(n, hkv, 128, generator=g).to(BF).to(DEV)


def build(hq: int, hkv: int, seqs: List[Seq], seed: int = 0):
    """(forked cache, call) -- the cache holds every Seq's OWN rows in its slot and NaN everywhere else: below a child's
    shared length and behind the live rows.  call: the slots, lengths, parents, shared lengths and new rows of the
    sequences in the call, in the order of `seqs`."""
    from cadence_rag_amd.encoder.generate import KvCache
    cache = KvCache(1, N_SLOTS, hkv, MAX_LEN, DEV)
    cache.k.fill_(float("nan"))
    cache.v.fill_(float("nan"))
    by_key: Dict[int, Seq] = {s.key: s for s in seqs}
    for s in seqs:
        lo, hi = s.shared, s.shared + s.private
        cache.k[0, s.slot, :, lo:hi] = _rows(s.key, 1, s.private, hkv).transpose(0, 1)
        cache.v[0, s.slot, :, lo:hi] = _rows(s.key, 2, s.private, hkv).transpose(0, 1)
        cache.lens[s.slot] = hi
        if s.parent is not None and s.shared:
            cache.parent[s.slot], cache.shared[s.slot] = by_key[s.parent].slot, s.shared
    live = [s for s in seqs if s.in_call]
    g = torch.Generator().manual_seed(seed)
    q_w = (1 + 0.1 * torch.randn(128, generator=g)).to(BF).to(DEV)
    k_w = (1 + 0.1 * torch.randn(128, generator=g)).to(BF).to(DEV)
    qkv = torch.stack([torch.randn((hq + 2 * hkv) * 128, generator=torch.Generator().manual_seed(1000 * s.key)).to(BF)
                       for s in live]).to(DEV)
    call = {"slots": [s.slot for s in live], "lens": [s.shared + s.private for s in live],
            "parents": [by_key[s.parent].slot if s.parent is not None else s.slot for s in live],
            "shared": [s.shared for s in live], "qkv": qkv, "q_w": q_w, "k_w": k_w, "keys": [s.key for s in live]}
    return cache, call


@pytest.fixture(scope="module")
def fixed():
    from cadence_rag_amd.encoder import ops
    return {"cos_sin": dp.rope_table(MAX_LEN, DEV),
            "ws": {hq: ops.decode_workspace(8, hq, MAX_LEN, DEV) for hq in (4, 8)}}


def private_copies(cache, call, hkv):
    """A cache whose slot b holds a private copy of the logical rows of sequence b of the call (KvCache.keys / .values
    of the forked cache: the parent's first `shared` rows, then the slot's own), NaN behind them."""
    from cadence_rag_amd.encoder.generate import KvCache
    ref = KvCache(1, len(call["slots"]), hkv, MAX_LEN, DEV)
    ref.k.fill_(float("nan"))
    ref.v.fill_(float("nan"))
    for b, (slot, m) in enumerate(zip(call["slots"], call["lens"])):
        keys, vals = cache.keys(0, slot), cache.values(0, slot)
        assert keys.shape[0] == m and not bool(torch.isnan(keys.float()).any()) and not bool(torch.isnan(vals.float()).any())
        ref.append_prefill(0, b, keys.clone(), vals.clone())
        ref.lens[b] = m
    return ref


def run_both(hq, hkv, seqs, fixed, seed=0):
    """The forked call and decode_attention over private copies: asserts equal output bits and equal appended rows, and
    that the forked call changed no other cache row.  Returns the outputs by Seq.key."""
    from cadence_rag_amd.encoder import ops
    cache, call = build(hq, hkv, seqs, seed)
    ref = private_copies(cache, call, hkv)
    n = len(call["slots"])
    want = torch.full((n, hq * 128), float("nan"), dtype=BF, device=DEV)
    got = torch.full((n, hq * 128), float("nan"), dtype=BF, device=DEV)
    args = (call["qkv"], call["q_w"], call["k_w"], fixed["cos_sin"])
    ops.decode_attention(*args, *ref.layer(0), list(range(n)), call["lens"], want, hq, hkv, dp.EPS, dp.SCALE, fixed["ws"][hq])
    k_before, v_before = cache.k.clone(), cache.v.clone()
    ops.decode_attention_shared(*args, *cache.layer(0), call["slots"], call["lens"], call["parents"], call["shared"], got,
                                hq, hkv, dp.EPS, dp.SCALE, fixed["ws"][hq])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want.float()).all())
    assert torch.equal(_bits(got), _bits(want)), (call["lens"], call["shared"], (got.float() - want.float()).abs().max())
    for b, (slot, m) in enumerate(zip(call["slots"], call["lens"])):
        assert torch.equal(_bits(cache.k[0, slot, :, m]), _bits(ref.k[0, b, :, m])), (b, slot, m)
        assert torch.equal(_bits(cache.v[0, slot, :, m]), _bits(ref.v[0, b, :, m])), (b, slot, m)
        cache.k[0, slot, :, m] = k_before[0, slot, :, m]
        cache.v[0, slot, :, m] = v_before[0, slot, :, m]
    assert torch.equal(_bits(cache.k), _bits(k_before)) and torch.equal(_bits(cache.v), _bits(v_before))
    return {key: got[b].clone() for b, key in enumerate(call["keys"])}


def group(first_key, parent_slot, child_slots, shared, privates, parent_private=0, parent_in_call=True):
    """A parent that owns shared + parent_private rows and one child per slot of child_slots, each sharing `shared`."""
    parent = Seq(first_key, parent_slot, shared + parent_private, in_call=parent_in_call)
    return [parent] + [Seq(first_key + 1 + i, slot, privates[i % len(privates)], parent=first_key, shared=shared)
                       for i, slot in enumerate(child_slots)]


@HEADS
def test_forked_call_equals_private_copies_bit_for_bit(gpu, heads, fixed):
    """Every shared length of the list, the private suffixes 0 / 1 / 127 / 128 ragged within the call, groups of 2, 3 and
    8 sequences -- the parent a member with rows of its own behind the shared ones, or outside the call."""
    hq, hkv = heads
    for i, shared in enumerate(SHARED):
        members = (2, 3, 8)[i % 3]
        privates = PRIVATE[i % 4:] + PRIVATE[:i % 4]
        if i % 2:     # the parent decodes along: members - 1 children
            seqs = group(1, 9, list(range(members - 1)), shared, privates, parent_private=PRIVATE[(i + 1) % 4])
        else:         # the parent finished earlier: `members` children
            seqs = group(1, 9, list(range(members)), shared, privates, parent_private=3, parent_in_call=False)
        run_both(hq, hkv, seqs, fixed, seed=shared)


@HEADS
def test_two_groups_and_an_unforked_sequence_in_one_call(gpu, heads, fixed):
    hq, hkv = heads
    a = group(10, 0, [3, 5], 257, [1, 127], parent_private=43)             # the parent in the call, 300 rows
    a[2].shared = 256                                                      # ragged shared lengths inside a group
    b = group(20, 7, [1, 2, 8], 200, [0, 128, 5], parent_in_call=False)    # the parent outside it
    b[3].shared = 130
    alone = [Seq(30, 4, 77)]
    run_both(hq, hkv, [a[1], b[1], a[0], alone[0], b[2], a[2], b[3], b[0]], fixed)


@HEADS
def test_a_parent_outside_the_call(gpu, heads, fixed):
    hq, hkv = heads
    run_both(hq, hkv, group(1, 6, [2, 0], 300, [128, 0], parent_private=17, parent_in_call=False), fixed)
    run_both(hq, hkv, group(1, 6, [2], 129, [1], parent_in_call=False), fixed)     # a single child: no group to share with


@HEADS
def test_other_orders_and_slots_give_the_same_bits(gpu, heads, fixed):
    hq, hkv = heads
    seqs = group(1, 9, [0, 1, 2], 257, [127, 0, 128], parent_private=1) + [Seq(7, 5, 140)]
    first = run_both(hq, hkv, seqs, fixed)
    moved = group(1, 2, [7, 4, 9], 257, [127, 0, 128], parent_private=1) + [Seq(7, 0, 140)]
    moved = [moved[3], moved[4], moved[1], moved[0], moved[2]]
    second = run_both(hq, hkv, moved, fixed)
    assert first.keys() == second.keys()
    for key in first:
        assert torch.equal(_bits(first[key]), _bits(second[key])), key
    alone = run_both(hq, hkv, [s for s in seqs if s.key in (1, 3)], fixed)          # ... and in a smaller call
    assert torch.equal(_bits(alone[3]), _bits(first[3])) and torch.equal(_bits(alone[1]), _bits(first[1]))


@HEADS
def test_forked_call_matches_the_fp32_formula(gpu, heads, fixed):
    """atol = rtol = 2e-2: the bar tests/test_decode_gpu.py sets for decode_attention against the same formula
    (test_decode_attention_matches_fp32_and_appends_exactly).  The reference reads the logical rows through KvCache."""
    from cadence_rag_amd.encoder import ops
    hq, hkv = heads
    cache, call = build(hq, hkv, group(1, 9, [0, 1, 2], 257, [127, 0, 128], parent_private=1), seed=5)
    case = dp.Case(hq, hkv, call["slots"], call["lens"], call["qkv"], call["q_w"], call["k_w"], fixed["cos_sin"], cache,
                   fixed["ws"][hq])
    ref = dp.reference(case, dp.rotated(case))
    got = torch.empty(4, hq * 128, dtype=BF, device=DEV)
    ops.decode_attention_shared(call["qkv"], call["q_w"], call["k_w"], fixed["cos_sin"], *cache.layer(0), call["slots"],
                                call["lens"], call["parents"], call["shared"], got, hq, hkv, dp.EPS, dp.SCALE, fixed["ws"][hq])
    err = float((got.float().cpu() - ref).abs().max())
    print(f"heads {heads}: max |d| = {err:.3e}")
    assert torch.allclose(got.float().cpu(), ref, atol=2e-2, rtol=2e-2), err


@HEADS
def test_degenerate_arguments_are_decode_attention(gpu, heads):
    """All parents equal to the slots -- with any shared length -- and shared lengths of 0 under any parent."""
    from cadence_rag_amd.encoder import ops
    hq, hkv = heads
    lens, slots = [300, 129, 0, 128], [5, 2, 7, 0]
    outs = []
    for parents, shared in ((None, None), (slots, [0] * 4), (slots, [300, 1, 0, 128]), ([1, 1, 1, 1], [0] * 4)):
        case = dp.make_case(hq, hkv, lens, slots, max_len=MAX_LEN, seed=3, device=DEV)
        out = torch.full((4, hq * 128), float("nan"), dtype=BF, device=DEV)
        args = (case.qkv_new, case.q_w, case.k_w, case.cos_sin, *case.cache.layer(0), slots, lens)
        if parents is None:
            ops.decode_attention(*args, out, hq, hkv, dp.EPS, dp.SCALE, case.workspace)
        else:
            ops.decode_attention_shared(*args, parents, shared, out, hq, hkv, dp.EPS, dp.SCALE, case.workspace)
        torch.cuda.synchronize()
        outs.append((out, case.cache.k.clone(), case.cache.v.clone()))
    for out, k, v in outs[1:]:
        assert torch.equal(_bits(out), _bits(outs[0][0]))
        assert torch.equal(_bits(k), _bits(outs[0][1])) and torch.equal(_bits(v), _bits(outs[0][2]))


def test_refusals_launch_nothing(gpu):
    from cadence_rag_amd import _native
    from cadence_rag_amd.encoder import ops
    case = dp.make_case(4, 2, [40, 9, 20], [0, 1, 2], n_slots=4, max_len=64, seed=1, device=DEV)
    qkv9 = torch.zeros(9, 8 * 128, dtype=BF, device=DEV)
    out = torch.full((9, 4 * 128), 7.0, dtype=BF, device=DEV)
    kc, vc = case.cache.layer(0)
    k_before, v_before = kc.clone(), vc.clone()

    def call(slots, lens, parents, shared, workspace=case.workspace):
        ops.decode_attention_shared(qkv9, case.q_w, case.k_w, case.cos_sin, kc, vc, slots, lens, parents, shared, out, 4, 2,
                                    dp.EPS, dp.SCALE, workspace)

    good = ([0, 1, 2], [40, 9, 20], [0, 0, 0], [0, 9, 20])
    refused = {
        # the checks of decode_attention
        "max_len": ([0, 1, 2], [40, 64, 20], [0, 0, 0], [0, 9, 20]),
        "cache length -1": ([0, 1, 2], [40, -1, 20], [0, 0, 0], [0, 0, 20]),
        "n_seqs": ([0, 1, 2, 3, 0, 1, 2, 3, 0], [1] * 9, [0] * 9, [0] * 9),
        "twice": ([0, 1, 1], [40, 9, 20], [0, 0, 0], [0, 9, 9]),
        "slot 4": ([0, 4, 2], [40, 9, 20], [0, 0, 0], [0, 9, 20]),
        # the fork checks
        "parent 4": ([0, 1, 2], [40, 9, 20], [0, 4, 0], [0, 9, 20]),
        "parent -1": ([0, 1, 2], [40, 9, 20], [0, 0, -1], [0, 9, 20]),
        "shared length -1": ([0, 1, 2], [40, 9, 20], [0, 0, 0], [0, -1, 20]),
        "shared length 10": ([0, 1, 2], [40, 9, 20], [0, 0, 0], [0, 10, 20]),          # beyond its own 9 rows
        "shares 20 rows of slot 1, which holds 9": ([0, 1, 2], [40, 9, 20], [0, 0, 1], [0, 9, 20]),
    }
    for match, args in refused.items():
        with pytest.raises(_native.NativeLibraryError, match=match):
            call(*args)
    with pytest.raises(_native.NativeLibraryError, match="workspace"):
        call(*good, workspace=case.workspace[:1024])
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and torch.equal(_bits(kc), _bits(k_before)) and torch.equal(_bits(vc), _bits(v_before))
    call([1, 2], [9, 20], [3, 3], [9, 20])       # a parent outside the call is allowed, whatever it holds
    call(*good)                                  # and the good call runs
    torch.cuda.synchronize()
    assert bool((out[3:] == 7.0).all())


# ---- the generator ----------------------------------------------------------------------------------------------
NEW = 12
TEXT = ("the customer called about a failed deployment of the api gateway and we saw ECONNRESET errors between the "
        "gateway and the billing service after the upgrade")
MORE = " and the agent confirmed the refund"


@pytest.fixture(scope="module")
def generator(tmp_path_factory):
    """The tiny checkpoint (2 random layers, byte-level BPE of 384 ids), its embedding table as the head."""
    from tiny_checkpoint import build_checkpoint
    from cadence_rag_amd.encoder.generate import Qwen3Generator
    from cadence_rag_amd.encoder.qwen3 import Qwen3Encoder
    root = tmp_path_factory.mktemp("fork_tiny")
    build_checkpoint(root)
    enc = Qwen3Encoder.from_pretrained(str(root), DEV, max_length=2048)
    return Qwen3Generator(enc, enc.embed, enc.tokenizer, max_context=2048, max_seqs=4, model_id="tiny")


@pytest.fixture(scope="module")
def prompt(generator):
    return generator.tokenizer.encode(TEXT, add_special_tokens=False)


def hand_loop(gen, prompt, n, new, params, streams, stop=(), g=None):
    """generate_samples without a fork: the prompt prefilled into slot 0, its rows copied into slots 1..n-1, the first
    tokens drawn on the replicated row, then step on the plain path (no slot is forked).  Returns (ids, accepted)."""
    from cadence_rag_amd import grammar
    from cadence_rag_amd.encoder import ops
    logits = gen.prefill([prompt]).repeat(n, 1)
    m = len(prompt)
    for s in range(1, n):
        gen.cache.k[:, s, :, :m] = gen.cache.k[:, 0, :, :m]
        gen.cache.v[:, s, :, :m] = gen.cache.v[:, 0, :, :m]
        gen.cache.lens[s] = m
    assert not any(gen.cache.forked(s) for s in range(n))
    stop = set(stop)
    if g is not None:
        tables = g.table.to(DEV) + g.dfa.to(DEV)
        state = torch.full((n,), int(g.dfa.start), dtype=torch.int32, device=DEV)
    out, accepted, live = [[] for _ in range(n)], [False] * n, list(range(n))
    for j in range(new):
        token = torch.empty(len(live), dtype=torch.int32, device=DEV)
        lanes = [streams[b] for b in live]
        if g is None:
            ops.sample(logits, params, j, lanes, token)
        else:
            idx = torch.tensor(live, dtype=torch.int64).to(DEV)
            cur = state.index_select(0, idx)
            bits = torch.empty(len(live), (g.table.vocab + 31) // 32, dtype=torch.int32, device=DEV)
            ops.grammar_argmax(logits, *tables, cur.clone(), token, allowed_bits=bits)
            ops.sample(logits, params, j, lanes, token, allowed_bits=bits)
            ops.grammar_advance(*tables[:5], cur, token)
            state.index_copy_(0, idx, cur)
        feed, keep = [], []
        for b, t in zip(live, token.tolist()):
            if g is not None and t >= 0 and g.table.kind[t] == grammar.KIND_STOP:
                accepted[b] = True
            elif t >= 0 and t not in stop:
                out[b].append(t)
                if len(out[b]) < new:
                    keep.append(b)
                    feed.append(t)
        live = keep
        if not live:
            break
        _, logits = gen.step(feed, slots=live)
        assert gen.last_path
    gen.live = []
    for s in range(1, n):
        gen.truncate(s, 0)
    return out, accepted


def _params():
    from cadence_rag_amd.sampling import SamplingParams
    return SamplingParams(0.9, top_k=40, seed=7)


def test_generate_samples_equals_the_hand_loop(gpu, generator, prompt, monkeypatch):
    from cadence_rag_amd.encoder import ops
    gen, streams = generator, [3, 0, 11, 5]
    assert gen.supports_samples is True
    calls = []
    real = ops.decode_attention_shared
    monkeypatch.setattr(ops, "decode_attention_shared", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    got = gen.generate_samples(prompt, 4, NEW, sampling=_params(), streams=streams)
    assert len(calls) == (NEW - 1) * gen.cfg.num_layers                   # every step of the forked slots went through it
    assert [len(o) for o in got] == [NEW] * 4 and len({tuple(o) for o in got}) == 4
    calls.clear()
    by_hand, _ = hand_loop(gen, prompt, 4, NEW, _params(), streams)
    assert not calls and got == by_hand
    assert gen.generate_samples(prompt, 4, NEW, sampling=_params()) == \
        gen.generate_samples(prompt, 4, NEW, sampling=_params(), streams=[0, 1, 2, 3])     # the default stream is i
    with pytest.raises(ValueError):
        gen.generate_samples(prompt, 5, NEW, sampling=_params())
    with pytest.raises(ValueError):
        gen.generate_samples(prompt, 0, NEW, sampling=_params())


def test_generate_samples_under_the_grammar_equals_the_hand_loop(gpu, generator, prompt):
    from cadence_rag_amd.grammar import TokenGrammar, citation_grammar
    gen, streams = generator, [3, 0, 11, 5]
    g = TokenGrammar(citation_grammar(["Q-12", "A-45"]), gen.token_table())
    got = gen.generate_samples(prompt, 4, NEW, gen.stop_ids(), grammar=g, sampling=_params(), streams=streams)
    got_accepted = gen.last_grammar["accepted"]
    by_hand, accepted = hand_loop(gen, prompt, 4, NEW, _params(), streams, gen.stop_ids(), g)
    print(f"by hand: {by_hand}, accepted {accepted}")
    assert got == by_hand and got_accepted == accepted and len(got_accepted) == 4 and any(by_hand)


def test_the_parent_stops_early_and_the_others_go_on(gpu, generator, prompt):
    gen, streams = generator, [3, 0, 11, 5]
    first = gen.generate_samples(prompt, 4, NEW, sampling=_params(), streams=streams)
    stop = first[0][2]                       # sample 0 emits it as its third token at the latest
    got = gen.generate_samples(prompt, 4, NEW, [stop], sampling=_params(), streams=streams)
    print(f"stop id {stop}: lengths {[len(o) for o in got]}")
    assert len(got[0]) <= 2 and got[0] == first[0][:len(got[0])]
    assert max(len(o) for o in got[1:]) > len(got[0]) + 1                  # they ran on the parent's rows after it ended
    by_hand, _ = hand_loop(gen, prompt, 4, NEW, _params(), streams, [stop])
    assert got == by_hand


def test_one_sample_is_generate(gpu, generator, prompt):
    gen = generator
    assert gen.generate_samples(prompt, 1, NEW) == gen.generate([prompt], NEW)
    assert gen.generate_samples(prompt, 1, NEW, sampling=_params(), streams=[6]) == \
        gen.generate([prompt], NEW, sampling=_params(), streams=[6])
    want = gen.generate([prompt], NEW)
    gen.prefill([prompt[:40]])
    assert gen.generate_samples(prompt, 1, NEW, reuse_prefix=True) == want
    assert gen.last_reuse == {"reused": [40], "computed": [len(prompt) - 40]}


def test_what_the_slots_hold_afterwards(gpu, generator, prompt):
    gen = generator
    out = gen.generate_samples(prompt, 4, NEW, sampling=_params())
    assert gen.cache.lens[1:] == [0, 0, 0] and not any(gen.cache.forked(s) for s in range(4)) and gen.live == []
    held = gen.cache.lens[0]
    assert held == len(prompt) + NEW - 1     # the budget ended the run: the last id was never fed, so it has no row
    assert gen.resident(0) == (list(prompt) + out[0])[:held]
    longer = list(prompt) + out[0] + gen.tokenizer.encode(MORE, add_special_tokens=False)
    want = gen.generate([longer], NEW)
    gen.generate_samples(prompt, 4, NEW, sampling=_params())
    assert gen.generate([longer], NEW, reuse_prefix=True) == want
    assert gen.last_reuse == {"reused": [held], "computed": [len(longer) - held]}
    # under reuse_prefix generate_samples plans slot 0 as generate does, and reports per sample
    gen.generate_samples(longer, 3, NEW, reuse_prefix=True, sampling=_params())
    assert gen.last_reuse == {"reused": [len(longer) - 1] * 3, "computed": [1] * 3}
    gen.truncate(0, 0)
    gen.generate_samples(longer, 3, NEW, reuse_prefix=True, sampling=_params())
    assert gen.last_reuse == {"reused": [0] * 3, "computed": [len(longer)] * 3}
    gen.generate_samples(longer, 3, NEW, sampling=_params())
    assert gen.last_reuse is None and gen.last_grammar is None


def test_a_plain_generate_never_reaches_the_shared_entry(gpu, generator, prompt, monkeypatch):
    from cadence_rag_amd.encoder import ops

    def boom(*a, **k):
        raise AssertionError("decode_attention_shared on unforked slots")

    gen = generator
    want = gen.generate([prompt, prompt[:50]], NEW)
    gen.generate_samples(prompt, 4, NEW, sampling=_params())
    monkeypatch.setattr(ops, "decode_attention_shared", boom)
    assert gen.generate([prompt, prompt[:50]], NEW) == want
    assert gen.generate([prompt, prompt[:50]], NEW, sampling=_params()) == \
        gen.generate([prompt, prompt[:50]], NEW, sampling=_params())
    with pytest.raises(AssertionError):
        gen.generate_samples(prompt, 2, NEW, sampling=_params())
    assert gen.cache.lens[1] == 0 and not gen.cache.forked(1)             # the children are emptied on the way out


def test_fork_rules(gpu, generator, prompt):
    gen = generator
    m = len(prompt)
    gen.prefill([prompt])
    gen.fork(0, [1, 2])
    assert gen.cache.lens[:3] == [m, m, m] and gen.cache.parent[1:3] == [0, 0] and gen.cache.shared[1:3] == [m, m]
    assert gen.resident(1) == [-1] * m
    assert torch.equal(gen.cache.keys(1, 2), gen.cache.keys(1, 0)) and torch.equal(gen.cache.values(0, 1), gen.cache.values(0, 0))
    with pytest.raises(ValueError, match="forked"):
        gen.extend([prompt[:5]], slots=[1])
    with pytest.raises(ValueError, match="parent of a live child"):
        gen.fork(3, [0])
    gen.step([5, 6], slots=[1, 2])                       # the children go on alone, the parent's rows stay
    assert gen.cache.lens[:3] == [m, m + 1, m + 1] and gen.cache.keys(0, 1).shape[0] == m + 1
    assert torch.equal(gen.cache.keys(0, 1)[:m], gen.cache.keys(0, 0))
    gen.truncate(1, 10)                                  # a child shortened below its shared length shares less
    assert gen.cache.shared[1] == 10 and gen.cache.lens[1] == 10 and gen.cache.forked(1)
    gen.truncate(0, m - 1)                               # the parent loses a row child 2 shares: child 2 is emptied
    assert gen.cache.lens[:3] == [m - 1, 10, 0] and not gen.cache.forked(2) and gen.cache.forked(1)
    gen.prefill([prompt[:20]])                           # a prefill into the parent empties the rest
    assert gen.cache.lens[:3] == [20, 0, 0] and not gen.cache.forked(1)
    gen.fork(0, [1])
    gen.prefill([prompt[:8]], slots=[1])                 # a prefill into a child unforks it
    assert not gen.cache.forked(1) and gen.cache.lens[:2] == [20, 8] and gen.resident(1) == list(prompt[:8])
    gen.live = []
