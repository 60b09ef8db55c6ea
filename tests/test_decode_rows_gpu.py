"""crag_enc_decode_attention_rows on the GPU: several new rows per sequence in one call, exact.

Every case compares the bits of `out` and of BOTH whole caches with the reference: the same rows fed one at a time
through ops.decode_attention (ops.decode_attention_shared for a forked sequence) on a clone of the cache.  The cache is
NaN wherever a row must not be read: at and beyond cache_len + new_len, and in a child's own slot below its shared
length.  Cache lengths and row counts put rows on both sides of a 128-key split edge."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import pytest
import torch

import decode_probes as dp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF = torch.bfloat16
MAX_LEN = 384
N_SLOTS = 10
HEADS = pytest.mark.parametrize("heads", [(8, 2), (4, 2)], ids=["group4", "group2"])
# (cache length, new rows): (126, 3) -- the third row opens a split whose only key this call appended
EDGES = [(0, 8), (1, 1), (126, 3), (127, 2), (128, 8), (255, 2), (300, 1)]


def _bits(t):
    return t.contiguous().view(torch.int16)


@dataclass
class Seq:
    """One sequence of a call: `key` seeds its data (the rows it owns and its new rows) whatever slot and place in the
    call it gets.  It holds `length` logical rows, the first `shared` of them in slot `parent` (None: not forked), and
    brings `rows` new ones.  rows == 0: not in the call (a finished parent, whose rows stay)."""
    key: int
    slot: int
    length: int
    rows: int
    parent: Optional[int] = None
    shared: int = 0


def _randn(key: int, what: int, *shape) -> torch.Tensor:
    return torch.randn(*shape, generator=torch.Generator().manual_seed(1000 * key + what)).to(BF).to(DEV)


@pytest.fixture(scope="module")
def fixed():
    from cadence_rag_amd.encoder import ops
    g = torch.Generator().manual_seed(11)
    return {"cos_sin": dp.rope_table(MAX_LEN, DEV),
            "q_w": (1 + 0.1 * torch.randn(128, generator=g)).to(BF).to(DEV),
            "k_w": (1 + 0.1 * torch.randn(128, generator=g)).to(BF).to(DEV),
            "ws": {hq: ops.decode_workspace(8, hq, MAX_LEN, DEV) for hq in (4, 8)}}


def build(hq: int, hkv: int, seqs: List[Seq]):
    """(cache, call): every Seq's OWN rows in its slot, NaN everywhere else; the call lists the Seqs with rows > 0."""
    from cadence_rag_amd.encoder.generate import KvCache
    cache = KvCache(1, N_SLOTS, hkv, MAX_LEN, DEV)
    cache.k.fill_(float("nan"))
    cache.v.fill_(float("nan"))
    for s in seqs:
        own = s.length - s.shared
        cache.k[0, s.slot, :, s.shared:s.length] = _randn(s.key, 1, own, hkv, 128).transpose(0, 1)
        cache.v[0, s.slot, :, s.shared:s.length] = _randn(s.key, 2, own, hkv, 128).transpose(0, 1)
    live = [s for s in seqs if s.rows]
    call = {"slots": [s.slot for s in live], "lens": [s.length for s in live], "news": [s.rows for s in live],
            "parents": [s.slot if s.parent is None else s.parent for s in live], "shared": [s.shared for s in live],
            "qkv": torch.cat([_randn(s.key, 3, s.rows, (hq + 2 * hkv) * 128) for s in live]),
            "keys": [s.key for s in live], "forked": any(s.parent is not None and s.shared for s in live)}
    return cache, call


def one_by_one(hq, hkv, cache, call, fixed):
    """The reference: every row of the call through the one-row entries, on a clone of the cache."""
    from cadence_rag_amd.encoder import ops
    kc, vc = cache.k[0].clone(), cache.v[0].clone()
    total = sum(call["news"])
    want = torch.full((total, hq * 128), float("nan"), dtype=BF, device=DEV)
    args = (fixed["q_w"], fixed["k_w"], fixed["cos_sin"], kc, vc)
    tail = (hq, hkv, dp.EPS, dp.SCALE, fixed["ws"][hq])
    row = 0
    for slot, m, r, parent, shared in zip(call["slots"], call["lens"], call["news"], call["parents"], call["shared"]):
        for i in range(r):
            if parent != slot and shared:
                ops.decode_attention_shared(call["qkv"][row:row + 1], *args, [slot], [m + i], [parent], [shared],
                                            want[row:row + 1], *tail)
            else:
                ops.decode_attention(call["qkv"][row:row + 1], *args, [slot], [m + i], want[row:row + 1], *tail)
            row += 1
    return want, kc, vc


def run_both(hq, hkv, seqs, fixed, forks=None):
    """The rows call against the reference: equal output bits, equal bits of both whole caches (the appended rows, and
    nothing else touched), finite outputs.  Returns the output rows by Seq.key."""
    from cadence_rag_amd.encoder import ops
    cache, call = build(hq, hkv, seqs)
    want, k_want, v_want = one_by_one(hq, hkv, cache, call, fixed)
    total = sum(call["news"])
    got = torch.full((total, hq * 128), float("nan"), dtype=BF, device=DEV)
    forks = call["forked"] if forks is None else forks
    ops.decode_attention_rows(call["qkv"], fixed["q_w"], fixed["k_w"], fixed["cos_sin"], *cache.layer(0), call["slots"],
                              call["lens"], call["news"], got, hq, hkv, dp.EPS, dp.SCALE, fixed["ws"][hq],
                              parents=call["parents"] if forks else None, shared_len=call["shared"] if forks else None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want.float()).all()) and bool(torch.isfinite(got.float()).all())
    what = (call["lens"], call["news"], call["shared"])
    assert torch.equal(_bits(got), _bits(want)), (what, (got.float() - want.float()).abs().max(dim=1).values)
    assert torch.equal(_bits(cache.k[0]), _bits(k_want)), what
    assert torch.equal(_bits(cache.v[0]), _bits(v_want)), what
    out, row = {}, 0
    for key, r in zip(call["keys"], call["news"]):
        out[key] = got[row:row + r].clone()
        row += r
    return out


@HEADS
@pytest.mark.parametrize("edge", EDGES, ids=[f"len{m}-rows{r}" for m, r in EDGES])
def test_rows_of_one_sequence_equal_successive_steps(gpu, heads, edge, fixed):
    hq, hkv = heads
    m, r = edge
    run_both(hq, hkv, [Seq(1, 3, m, r)], fixed)
    run_both(hq, hkv, [Seq(1, 3, m, r)], fixed, forks=True)     # the fork arrays given, nobody forked


@HEADS
def test_mixed_row_counts_over_three_slots(gpu, heads, fixed):
    hq, hkv = heads
    run_both(hq, hkv, [Seq(1, 7, 127, 1), Seq(2, 0, 254, 3), Seq(3, 4, 30, 4)], fixed)


@HEADS
def test_eight_sequences_of_one_row_are_decode_attention(gpu, heads, fixed):
    from cadence_rag_amd.encoder import ops
    hq, hkv = heads
    lens = [0, 1, 127, 128, 129, 255, 256, 300]
    seqs = [Seq(10 + b, (3 * b + 1) % 8, m, 1) for b, m in enumerate(lens)]
    got = run_both(hq, hkv, seqs, fixed)
    cache, call = build(hq, hkv, seqs)
    want = torch.full((8, hq * 128), float("nan"), dtype=BF, device=DEV)
    ops.decode_attention(call["qkv"], fixed["q_w"], fixed["k_w"], fixed["cos_sin"], *cache.layer(0), call["slots"],
                         call["lens"], want, hq, hkv, dp.EPS, dp.SCALE, fixed["ws"][hq])
    for b, s in enumerate(seqs):
        assert torch.equal(_bits(got[s.key][0]), _bits(want[b])), s


@HEADS
def test_a_sequences_bits_do_not_depend_on_the_call(gpu, heads, fixed):
    hq, hkv = heads
    alone = run_both(hq, hkv, [Seq(5, 2, 126, 3)], fixed)
    last = run_both(hq, hkv, [Seq(6, 0, 300, 1), Seq(7, 9, 0, 4), Seq(5, 6, 126, 3)], fixed)
    assert torch.equal(_bits(alone[5]), _bits(last[5]))


@HEADS
def test_forked_sequences(gpu, heads, fixed):
    """A child (130 shared rows, 133 in all, 3 new) with its parent in the call (2 new rows behind 131); a child whose
    parent is outside the call; both in one call with an unforked sequence.  The children's own slots are NaN below
    their shared lengths."""
    hq, hkv = heads
    parent, child = Seq(1, 4, 131, 2), Seq(2, 1, 133, 3, parent=4, shared=130)
    both = run_both(hq, hkv, [child, parent], fixed)
    run_both(hq, hkv, [Seq(1, 4, 131, 0), child], fixed)                       # the parent outside the call
    run_both(hq, hkv, [Seq(1, 4, 300, 0), Seq(3, 8, 300, 4, parent=4, shared=300)], fixed)   # no row of its own yet
    mixed = run_both(hq, hkv, [Seq(9, 0, 127, 2), parent, Seq(4, 6, 257, 1, parent=5, shared=256), child,
                               Seq(8, 5, 256, 0)], fixed)
    assert torch.equal(_bits(both[2]), _bits(mixed[2])) and torch.equal(_bits(both[1]), _bits(mixed[1]))


def test_refusals_launch_nothing(gpu, fixed):
    from cadence_rag_amd import _native
    from cadence_rag_amd.encoder import ops
    hq, hkv = 4, 2
    cache, _ = build(hq, hkv, [Seq(1, 0, 40, 1), Seq(2, 1, 9, 1), Seq(3, 2, 20, 1)])
    kc, vc = cache.k[0, :4, :, :64].contiguous(), cache.v[0, :4, :, :64].contiguous()    # 4 slots of 64 rows
    qkv = torch.zeros(16, (hq + 2 * hkv) * 128, dtype=BF, device=DEV)
    out = torch.full((16, hq * 128), 7.0, dtype=BF, device=DEV)
    k_before, v_before = kc.clone(), vc.clone()
    ws = fixed["ws"][hq]

    def call(slots, lens, news, parents=None, shared=None, workspace=ws):
        ops.decode_attention_rows(qkv, fixed["q_w"], fixed["k_w"], fixed["cos_sin"], kc, vc, slots, lens, news, out, hq,
                                  hkv, dp.EPS, dp.SCALE, workspace, parents=parents, shared_len=shared)

    good = ([0, 1, 2], [40, 9, 20], [2, 1, 5], [0, 0, 0], [0, 9, 20])
    refused = {
        "brings 0 new rows": ([0, 1, 2], [40, 9, 20], [2, 0, 5]),
        "brings -1 new rows": ([0, 1, 2], [40, 9, 20], [2, -1, 5]),
        "at most 8": ([0, 1, 2], [40, 9, 20], [2, 2, 5]),
        "at most 8 new": ([0], [0], [9]),
        "do not fit": ([0, 1, 2], [62, 9, 20], [3, 1, 4]),                   # 62 + 3 > max_len 64
        "negative": ([0, 1, 2], [40, -1, 20], [2, 1, 5]),
        "n_seqs": ([0, 1, 2, 3, 0, 1, 2, 3, 0], [1] * 9, [1] * 9),
        "twice": ([0, 1, 1], [40, 9, 20], [2, 1, 5]),
        "slot 4": ([0, 4, 2], [40, 9, 20], [2, 1, 5]),
        "parent 4": ([0, 1, 2], [40, 9, 20], [2, 1, 5], [0, 4, 0], [0, 9, 20]),
        "parent -1": ([0, 1, 2], [40, 9, 20], [2, 1, 5], [0, 0, -1], [0, 9, 20]),
        "shared length -1": ([0, 1, 2], [40, 9, 20], [2, 1, 5], [0, 0, 0], [0, -1, 20]),
        "shared length 10": ([0, 1, 2], [40, 9, 20], [2, 1, 5], [0, 0, 0], [0, 10, 20]),
        # slot 1 is in the call with 9 rows: rows 9.. are appended during it
        "shares 20 rows of slot 1, which holds 9": ([0, 1, 2], [40, 9, 20], [2, 1, 5], [0, 0, 1], [0, 9, 20]),
    }
    for match, args in refused.items():
        with pytest.raises(_native.NativeLibraryError, match=match):
            call(*args)
    with pytest.raises(_native.NativeLibraryError, match="workspace"):
        call(*good, workspace=ws[:1024])
    with pytest.raises(ValueError):
        call(*good[:4])                                                     # parents without shared lengths
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and torch.equal(_bits(kc), _bits(k_before)) and torch.equal(_bits(vc), _bits(v_before))
    call(*good)                                                             # and the good call runs
    torch.cuda.synchronize()
    assert bool((out[8:] == 7.0).all()) and bool(torch.isfinite(out[:8].float()).all())
