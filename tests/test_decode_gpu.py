"""crag_enc_decode_attention and crag_enc_lm_head on the GPU: against the fp32 formula over ragged caches, the append bit
for bit against crag_enc_qk_norm_rope, exact one-key probes over every position of a 300-key cache, independence of the
output bits from the batch and the slot, the argument checks, and the full-vocabulary head with its greedy token."""
from __future__ import annotations

import ctypes

import pytest
import torch

import decode_probes as dp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF = torch.bfloat16


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("heads", [(4, 2), (8, 2)], ids=["group2", "group4"])
def test_decode_attention_matches_fp32_and_appends_exactly(gpu, heads):
    """Every length of dp.LENGTHS (the issue's list plus the values around the 16-key pass and the 128-key split), three
    ragged sequences per call in non-adjacent slots; cache rows behind the live ones are NaN.  atol = rtol = 2e-2, the
    bar of the flash kernels against the same formula (test_rerank_gpu.py).  After the call the row `len` of every slot
    holds the bits crag_enc_qk_norm_rope writes and the raw value; every other cache row is unchanged."""
    hq, hkv = heads
    lengths = dp.LENGTHS
    for i in range(0, len(lengths), 3):
        lens = [lengths[(i + d) % len(lengths)] for d in range(3)]
        case = dp.make_case(hq, hkv, lens, slots=[6, 1, 4], seed=17 * i + hq, device=DEV)
        rot = dp.rotated(case)
        ref = dp.reference(case, rot)
        k_before, v_before = case.cache.k.clone(), case.cache.v.clone()
        got = dp.run(case).float().cpu()
        assert torch.isfinite(got).all(), lens
        err = float((got - ref).abs().max())
        print(f"heads {heads} lens {lens}: max |d| = {err:.3e}")
        assert torch.allclose(got, ref, atol=2e-2, rtol=2e-2), (heads, lens, err)
        for b, (slot, m) in enumerate(zip(case.slots, lens)):
            want_k = rot[b, hq * 128: (hq + hkv) * 128].view(hkv, 128)
            want_v = case.qkv_new[b, (hq + hkv) * 128:].view(hkv, 128)
            assert case.cache.lens[slot] == m + 1
            assert torch.equal(_bits(case.cache.keys(0, slot)[m]), _bits(want_k)), (lens, b)
            assert torch.equal(_bits(case.cache.values(0, slot)[m]), _bits(want_v)), (lens, b)
            # ... and nothing else moved: put the old row back and compare the whole arrays, NaNs included
            case.cache.keys(0, slot)[m] = float("nan")
            case.cache.values(0, slot)[m] = float("nan")
        assert torch.equal(_bits(case.cache.k), _bits(k_before)) and torch.equal(_bits(case.cache.v), _bits(v_before))


@pytest.mark.parametrize("heads", [(4, 2), (8, 2)], ids=["group2", "group4"])
def test_one_key_probes_are_exact(gpu, heads):
    """Key j of a 300-key cache is the only one that weighs: the output is V[j] bit for bit, for every j including the
    new token's own position (eight probes per call)."""
    hq, hkv = heads
    n_keys = 300
    for j0 in range(0, n_keys, 8):
        js = list(range(j0, min(j0 + 8, n_keys)))
        case, want = dp.one_key_case(hq, hkv, js, n_keys, seed=j0 + hq, device=DEV)
        got = dp.run(case)
        assert torch.equal(_bits(got), _bits(want)), (heads, js, (got.float() - want.float()).abs().max())


@pytest.mark.parametrize("heads", [(4, 2), (8, 2)], ids=["group2", "group4"])
def test_output_bits_do_not_depend_on_the_batch_or_the_slot(gpu, heads):
    hq, hkv = heads
    lens, slots = [700, 129, 33], [5, 2, 7]
    outs = []
    for _ in range(2):                                   # two runs of the batch of three
        case = dp.make_case(hq, hkv, lens, slots, seed=3, device=DEV)
        outs.append(dp.run(case))
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    for b in range(3):                                   # each sequence alone ...
        case = dp.make_case(hq, hkv, lens, slots, seed=3, device=DEV)
        assert torch.equal(_bits(dp.run(case, [b])[0]), _bits(outs[0][b])), b
    # ... and alone in another slot: the same keys, values and new row moved to slot 0
    case = dp.make_case(hq, hkv, lens, slots, seed=3, device=DEV)
    moved = dp.make_case(hq, hkv, [lens[0]], [0], seed=99, device=DEV)
    moved.cache.append_prefill(0, 0, case.cache.keys(0, slots[0]).clone(), case.cache.values(0, slots[0]).clone())
    moved.qkv_new, moved.q_w, moved.k_w = case.qkv_new[:1].contiguous(), case.q_w, case.k_w
    assert torch.equal(_bits(dp.run(moved)[0]), _bits(outs[0][0]))


def test_argument_checks_enqueue_nothing(gpu):
    from cadence_rag_amd import _native
    lib = _native.load()
    case = dp.make_case(4, 2, [5, 9, 2], [0, 1, 2], n_slots=4, max_len=64, seed=1, device=DEV)
    qkv9 = torch.zeros(9, 8 * 128, dtype=BF, device=DEV)
    out = torch.full((9, 4 * 128), 7.0, dtype=BF, device=DEV)
    kc, vc = case.cache.layer(0)
    k_before = kc.clone()

    def call(slots, lens, n=None, qkv=qkv9, out_t=out):
        n = len(slots) if n is None else n
        a = (ctypes.c_int32 * 9)(*(list(slots) + [0] * (9 - len(slots))))
        b = (ctypes.c_int32 * 9)(*(list(lens) + [0] * (9 - len(lens))))
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731
        return lib.crag_enc_decode_attention(p(qkv), p(case.q_w), p(case.k_w), p(case.cos_sin), 64, p(kc), p(vc), 4, 64, a, b,
                                             n, 4, 2, 1e-6, dp.SCALE, p(case.workspace), case.workspace.numel(), p(out_t),
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    assert call([0, 1, 2], [5, 64, 2]) == -1 and "max_len" in _native.last_error()
    assert call([0, 1, 2], [5, -1, 2]) == -1
    assert call([0, 1, 2, 3, 0, 1, 2, 3, 0], [1] * 9) == -1 and "n_seqs" in _native.last_error()
    assert call([0, 1, 1], [5, 9, 2]) == -1 and "twice" in _native.last_error()
    assert call([0, 4, 1], [5, 9, 2]) == -1
    assert call([0, 1, 2], [5, 9, 2], qkv=None) == -1 and "NULL" in _native.last_error()
    assert call([0, 1, 2], [5, 9, 2], out_t=None) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and torch.equal(_bits(kc), _bits(k_before))
    assert call([0, 1, 2], [5, 9, 2]) == 0                 # the same call with good arguments runs
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:3].float()).all()) and bool((out[3:] == 7.0).all())


# ---- lm_head ----------------------------------------------------------------------------------------------------
def _lm_reference(hs, delta, w, lm, eps):
    x = (hs.float() + delta.float()).to(BF).float() if delta is not None else hs.float()
    normed = (w.float() * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)).to(BF).float()).to(BF).float()
    return normed.cpu(), normed.cpu() @ lm.float().cpu().T


def _lowest_argmax(row, banned=()):
    row = row.clone()
    for b in banned:
        row[b] = float("-inf")
    return int((row == row.max()).nonzero()[0])


@pytest.mark.parametrize("vocab", [300, 4099])
@pytest.mark.parametrize("rows", [1, 5])
def test_lm_head_matches_torch_and_picks_the_lowest_maximum(gpu, vocab, rows):
    """Logits against the torch formula at rerank_head's tolerances (atol 2e-4, rtol 1e-4); the token is the lowest-id
    argmax of the kernel's own logits, exactly; the last row has two planted equal maxima and a banned larger one."""
    from cadence_rag_amd.encoder import ops
    g = torch.Generator().manual_seed(vocab + rows)
    hidden, eps = 2560, 1e-6
    hs = (torch.randn(rows, hidden, generator=g)).to(BF).to(DEV)
    delta = (torch.randn(rows, hidden, generator=g) * 0.5).to(BF).to(DEV)
    w = (1 + 0.1 * torch.randn(hidden, generator=g)).to(BF).to(DEV)
    lm = (torch.randn(vocab, hidden, generator=g) * 0.05).to(BF)
    normed, _ = _lm_reference(hs, delta, w, lm.to(DEV), eps)
    a, b, c = vocab - 1, 41, 150          # b < a: the lowest id must win; c is larger still, and banned
    lm[a] = lm[b] = (normed[-1] * 0.05).to(BF)
    lm[c] = (normed[-1] * 0.1).to(BF)
    lm = lm.to(DEV)
    _, want = _lm_reference(hs, delta, w, lm, eps)
    for banned in (None, [c], [c, b], [7, c, 299]):
        logits = torch.full((rows, vocab), float("nan"), dtype=torch.float32, device=DEV)
        token = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
        bt = None if banned is None else torch.tensor(banned, dtype=torch.int32, device=DEV)
        ops.lm_head(hs, w, lm, logits, token, eps, delta=delta, banned=bt)
        got, tok = logits.cpu(), token.cpu().tolist()
        err = float((got - want).abs().max())
        print(f"vocab {vocab} rows {rows} banned {banned}: max |dlogit| = {err:.3e}")
        assert torch.allclose(got, want, atol=2e-4, rtol=1e-4), err
        assert tok == [_lowest_argmax(got[r], banned or ()) for r in range(rows)], (tok, banned)
        assert float(got[-1, a]) == float(got[-1, b])                       # the planted tie is a tie in the kernel's logits
        assert tok[-1] == {None: c, 1: b, 2: a, 3: b}[banned and len(banned)]
    # without delta; a tied model passes its embedding table: same entry
    logits = torch.empty(rows, vocab, dtype=torch.float32, device=DEV)
    token = torch.empty(rows, dtype=torch.int32, device=DEV)
    ops.lm_head(hs, w, lm, logits, token, eps)
    _, want = _lm_reference(hs, None, w, lm, eps)
    assert torch.allclose(logits.cpu(), want, atol=2e-4, rtol=1e-4)
    assert token.cpu().tolist() == [_lowest_argmax(logits.cpu()[r]) for r in range(rows)]


def test_lm_head_argument_checks(gpu):
    from cadence_rag_amd import _native
    from cadence_rag_amd.encoder import ops
    hs = torch.zeros(9, 256, dtype=BF, device=DEV)
    w = torch.ones(256, dtype=BF, device=DEV)
    lm = torch.zeros(300, 256, dtype=BF, device=DEV)
    logits = torch.full((9, 300), 7.0, dtype=torch.float32, device=DEV)
    token = torch.full((9,), -7, dtype=torch.int32, device=DEV)
    with pytest.raises(_native.NativeLibraryError, match="n_rows"):
        ops.lm_head(hs, w, lm, logits, token, 1e-6)
    banned = torch.zeros(65, dtype=torch.int32, device=DEV)
    with pytest.raises(_native.NativeLibraryError, match="n_banned"):
        ops.lm_head(hs[:2], w, lm, logits[:2], token[:2], 1e-6, banned=banned)
    torch.cuda.synchronize()
    assert bool((logits == 7.0).all()) and bool((token == -7).all())
