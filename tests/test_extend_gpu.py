"""crag_enc_extend_attention on the GPU: against the fp32 formula over ragged caches and ragged suffixes with the
appended rows bit for bit against crag_enc_qk_norm_rope, exact one-key probes over every key visible to the edge rows of
every query block, independence of the bits from the batch and the slot, agreement with decode_attention and with
itself in two calls, and the argument checks."""
from __future__ import annotations

import ctypes

import pytest
import torch

import decode_probes as dp
import extend_probes as ep

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF = torch.bfloat16
HEADS = pytest.mark.parametrize("heads", [(4, 2), (8, 2)], ids=["group2", "group4"])


def _bits(t):
    return t.contiguous().view(torch.int16)


def _appended(case, b, m, n):
    """(keys, values) [n, hkv, 128] that sequence b's slot holds at rows m .. m + n - 1."""
    slot = case.slots[b]
    return case.cache.keys(0, slot)[m:m + n], case.cache.values(0, slot)[m:m + n]


@HEADS
def test_extend_matches_fp32_and_appends_exactly(gpu, heads):
    """ep.pairs(): the issue's cache and suffix lengths (which hold the values around the 32-row query block and the
    32-key tile: 31 / 32 / 33 / 63 / 64 / 65) and the lengths around the 512-key split and the 512-row limit of
    splitting, as ragged batches of three in non-adjacent slots; every cache row behind the live ones is NaN.  atol = rtol = 2e-2, the bar of the flash and decode kernels against the same formula.  After
    the call the rows len .. len + new - 1 of every slot hold the bits crag_enc_qk_norm_rope writes and the raw values;
    every other cache byte is unchanged; the rows of out behind the last sequence keep their marker."""
    hq, hkv = heads
    pairs = ep.pairs()
    for i in range(0, len(pairs), 3):
        lens, news = [p[0] for p in pairs[i:i + 3]], [p[1] for p in pairs[i:i + 3]]
        case = ep.make_case(hq, hkv, lens, news, slots=[6, 1, 4], seed=17 * i + hq, device=DEV)
        rot = ep.rotated(case)
        ref = ep.reference(case, rot)
        k_before, v_before = case.cache.k.clone(), case.cache.v.clone()
        out = ep.run(case)
        got = out[:-ep.PAD].float().cpu()
        assert bool((out[-ep.PAD:] == ep.MARK).all()), (lens, news)
        assert torch.isfinite(got).all(), (lens, news)
        err = float((got - ref).abs().max())
        print(f"heads {heads} cache {lens} new {news}: max |d| = {err:.3e}")
        assert torch.allclose(got, ref, atol=2e-2, rtol=2e-2), (heads, lens, news, err)
        for b, (slot, m, n) in enumerate(zip(case.slots, lens, news)):
            a = case.row0(b)
            want_k = rot[a:a + n, hq * 128: (hq + hkv) * 128].view(n, hkv, 128)
            want_v = case.qkv_new[a:a + n, (hq + hkv) * 128:].view(n, hkv, 128)
            assert case.cache.lens[slot] == m + n
            got_k, got_v = _appended(case, b, m, n)
            assert torch.equal(_bits(got_k), _bits(want_k)), (lens, news, b)
            assert torch.equal(_bits(got_v), _bits(want_v)), (lens, news, b)
            # ... and nothing else moved: put the old rows back and compare the whole arrays, NaNs included
            got_k.fill_(float("nan"))
            got_v.fill_(float("nan"))
        assert torch.equal(_bits(case.cache.k), _bits(k_before)) and torch.equal(_bits(case.cache.v), _bits(v_before))


@HEADS
def test_one_key_probes_are_exact(gpu, heads):
    """120 cached + 80 new rows = 200 keys (query blocks of 32, 32 and a partial 16).  For r = the first and the last
    row of every block, every key j <= 120 + r visible to it (cached keys, new keys, and its own diagonal key) in turn
    is the only one that weighs: out[r] is V[j] bit for bit.  Planted one past the row's own position the key must not
    weigh: out[r] is not its value."""
    hq, hkv = heads
    m, n = 120, 80
    edge_rows = [0, ep.BLOCK - 1, ep.BLOCK, 2 * ep.BLOCK - 1, 2 * ep.BLOCK, n - 1]
    probes = [(r, j) for r in edge_rows for j in range(m + r + 1)]
    for i in range(0, len(probes), 8):
        chunk = probes[i:i + 8]
        case, rows, want = ep.one_key_case(hq, hkv, chunk, m, n, seed=i + hq, device=DEV)
        got = ep.run(case).index_select(0, rows)
        assert torch.equal(_bits(got), _bits(want)), (heads, chunk, (got.float() - want.float()).abs().max())
    hidden = [(r, m + r + 1) for r in edge_rows if r + 1 < n]
    case, rows, value = ep.one_key_case(hq, hkv, hidden, m, n, seed=5, device=DEV)
    got = ep.run(case).index_select(0, rows)
    assert torch.isfinite(got.float()).all()
    for b in range(len(hidden)):
        assert not torch.equal(_bits(got[b]), _bits(value[b])), (heads, hidden[b])


@HEADS
def test_one_key_probes_across_the_key_split(gpu, heads):
    """SPLIT - 12 cached + 40 new rows: both query blocks have two key splits, and the first rows of the first block see
    no key of the second split at all.  For r = the edge rows of the blocks and the rows whose own key is the last of
    split 0 and the first of split 1, every visible key j of the first 40 and from SPLIT - 42 on: out[r] is V[j] bit for
    bit through the partials and the combine."""
    hq, hkv = heads
    m, n = ep.SPLIT - 12, 40
    edge_rows = [0, 11, 12, ep.BLOCK - 1, ep.BLOCK, n - 1]
    probes = [(r, j) for r in edge_rows for j in range(m + r + 1) if j < 40 or j >= ep.SPLIT - 42]
    for i in range(0, len(probes), 8):
        chunk = probes[i:i + 8]
        case, rows, want = ep.one_key_case(hq, hkv, chunk, m, n, seed=i + hq, device=DEV)
        got = ep.run(case).index_select(0, rows)
        assert torch.equal(_bits(got), _bits(want)), (heads, chunk, (got.float() - want.float()).abs().max())


@HEADS
def test_bits_do_not_depend_on_the_batch_or_the_slot(gpu, heads):
    hq, hkv = heads
    lens, news, slots = [700, 129, 33], [65, 32, 1], [5, 2, 7]

    def state(case, b, out, a):
        k, v = _appended(case, b, lens[b], news[b])
        return [_bits(out[a:a + news[b]]), _bits(k), _bits(v)]

    runs = []
    for _ in range(2):                                   # two runs of the batch of three
        case = ep.make_case(hq, hkv, lens, news, slots, seed=3, device=DEV)
        out = ep.run(case)
        runs.append([state(case, b, out, case.row0(b)) for b in range(3)])
    for b in range(3):
        assert all(torch.equal(x, y) for x, y in zip(runs[0][b], runs[1][b])), b
    for b in range(3):                                   # each sequence alone ...
        case = ep.make_case(hq, hkv, lens, news, slots, seed=3, device=DEV)
        out = ep.run(case, [b])
        assert all(torch.equal(x, y) for x, y in zip(state(case, b, out, 0), runs[0][b])), b
    # ... and alone in another slot: the same keys, values and new rows moved to slot 0
    case = ep.make_case(hq, hkv, lens, news, slots, seed=3, device=DEV)
    moved = ep.make_case(hq, hkv, [lens[0]], [news[0]], [0], seed=99, device=DEV)
    moved.cache.append_prefill(0, 0, case.cache.keys(0, slots[0]).clone(), case.cache.values(0, slots[0]).clone())
    moved.qkv_new, moved.q_w, moved.k_w = case.qkv_new[:news[0]].contiguous(), case.q_w, case.k_w
    out = ep.run(moved)
    k, v = moved.cache.keys(0, 0)[lens[0]:], moved.cache.values(0, 0)[lens[0]:]
    assert all(torch.equal(x, y) for x, y in zip([_bits(out[:news[0]]), _bits(k), _bits(v)], runs[0][0]))


@HEADS
def test_one_new_row_agrees_with_decode_attention(gpu, heads):
    """new_len = 1 is decode's case: outputs within 2e-2 (both kernels' bar against the fp32 formula), the appended row
    bit-equal."""
    hq, hkv = heads
    lens, slots = [700, 129, 33], [5, 2, 7]
    dec = dp.make_case(hq, hkv, lens, slots, max_len=1111, seed=11, device=DEV)
    ext = ep.make_case(hq, hkv, lens, [1, 1, 1], slots, seed=12, device=DEV)
    ext.cache.k.copy_(dec.cache.k)
    ext.cache.v.copy_(dec.cache.v)
    ext.qkv_new, ext.q_w, ext.k_w = dec.qkv_new, dec.q_w, dec.k_w
    want = dp.run(dec).float()
    got = ep.run(ext)[:3].float()
    print(f"heads {heads}: extend vs decode max |d| = {float((got - want).abs().max()):.3e}")
    assert torch.allclose(got, want, atol=2e-2, rtol=2e-2)
    for slot, m in zip(slots, lens):
        assert torch.equal(_bits(ext.cache.keys(0, slot)[m]), _bits(dec.cache.keys(0, slot)[m]))
        assert torch.equal(_bits(ext.cache.values(0, slot)[m]), _bits(dec.cache.values(0, slot)[m]))


@HEADS
def test_one_call_agrees_with_two(gpu, heads):
    """100 rows in one call against 33 + 67 in two: the same cache bits, the outputs of all 100 rows within 2e-2 (a row
    falls into another query block, its keys into the same tiles)."""
    hq, hkv = heads
    one = ep.make_case(hq, hkv, [45], [100], [3], seed=21, device=DEV)
    two = ep.make_case(hq, hkv, [45], [100], [3], seed=21, device=DEV)
    whole = ep.run(one)[:100].float()
    parts = torch.cat([ep.run(two, part=(0, 33))[:33], ep.run(two, part=(33, 67))[:67]]).float()
    assert one.cache.lens[3] == two.cache.lens[3] == 145
    assert torch.equal(_bits(one.cache.k), _bits(two.cache.k)) and torch.equal(_bits(one.cache.v), _bits(two.cache.v))
    print(f"heads {heads}: one call vs two max |d| = {float((whole - parts).abs().max()):.3e}")
    assert torch.allclose(whole, parts, atol=2e-2, rtol=2e-2)


def test_argument_checks_enqueue_nothing(gpu):
    from cadence_rag_amd import _native
    lib = _native.load()
    case = ep.make_case(4, 2, [5, 9, 2], [3, 1, 4], [0, 1, 2], n_slots=4, max_len=64, seed=1, device=DEV)
    qkv = torch.zeros(64, 8 * 128, dtype=BF, device=DEV)
    out = torch.full((64, 4 * 128), 7.0, dtype=BF, device=DEV)
    kc, vc = case.cache.layer(0)
    k_before, v_before = kc.clone(), vc.clone()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def call(slots, lens, news, n=None, qkv_t=qkv, out_t=out, hq=4, hkv=2, max_pos=64, ws_bytes=None, ws_off=0):
        n = len(slots) if n is None else n
        arr = lambda xs: (ctypes.c_int32 * 9)(*(list(xs) + [0] * (9 - len(xs))))   # noqa: E731
        ws = ctypes.c_void_p(case.workspace.data_ptr() + ws_off)
        return lib.crag_enc_extend_attention(p(qkv_t), p(case.q_w), p(case.k_w), p(case.cos_sin), max_pos, p(kc), p(vc), 4, 64,
                                             arr(slots), arr(lens), arr(news), n, hq, hkv, 1e-6, dp.SCALE, ws,
                                             case.workspace.numel() if ws_bytes is None else ws_bytes, p(out_t),
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    good = ([0, 1, 2], [5, 9, 2], [3, 1, 4])
    assert call([0, 1, 2], [5, 62, 2], [3, 3, 4]) == -1 and "max_len" in _native.last_error()
    assert call(*good, max_pos=9) == -1 and "RoPE" in _native.last_error()
    assert call([0, 1, 2], [5, -1, 2], [3, 1, 4]) == -1 and "negative" in _native.last_error()
    assert call([0, 1, 2], [5, 9, 2], [3, 0, 4]) == -1 and "new_len" in _native.last_error()
    assert call([0, 1, 2, 3, 0, 1, 2, 3, 0], [1] * 9, [1] * 9) == -1 and "n_seqs" in _native.last_error()
    assert call([], [], [], n=0) == -1 and "n_seqs" in _native.last_error()
    assert call([0, 1, 1], *good[1:]) == -1 and "twice" in _native.last_error()
    assert call([0, 4, 1], *good[1:]) == -1 and "slot" in _native.last_error()
    assert call(*good, hq=6, hkv=2) == -1 and "hq / hkv" in _native.last_error()
    assert call(*good, qkv_t=None) == -1 and "NULL" in _native.last_error()
    assert call(*good, out_t=None) == -1 and "NULL" in _native.last_error()
    assert call(*good, ws_off=8) == -1 and "aligned" in _native.last_error()
    assert call(*good, ws_bytes=8 * 4 * 256 - 1) == _native.CRAG_E2BIG and "workspace" in _native.last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert torch.equal(_bits(kc), _bits(k_before)) and torch.equal(_bits(vc), _bits(v_before))
    assert call(*good) == 0                                # the same call with good arguments runs
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:8].float()).all()) and bool((out[8:] == 7.0).all())
