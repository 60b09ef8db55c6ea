"""One-key probes through the attention kernels (construction, references and guards: tests/attention_probes.py; the
guards of every case here are proven on the CPU by tests/test_attention_probes_host.py and asserted again below).

A selection probe's output must equal V[target] bit for bit, for every row and head; a lure probe's output must be the
fp32 reference's soft mixture at atol = rtol = 2e-2 -- a forbidden key let in would miss that bar tenfold.  Each launch
builds V^T with crag_enc_v_transpose or crag_enc_qk_rope_vt first, as the forward does, so the PV slot order is probed too.

Kernels reached: crag_enc_attention -> attention_kernel<1, false> (g1), <2, false> (g2), <4, false> (g4-single),
attention_pair_kernel<4> (g4-pair*), <8> (g8-pair); crag_enc_attention_prefixed -> attention_kernel<2, true> (g2-p*),
<4, true> (g4-p*); the three fused entry points -> small_attn_kernel<1> (longest sequence <= 16) and <2>, as one block,
one block per sequence and over split-K partial tiles."""
from __future__ import annotations

import pytest
import torch

import attention_probes as ap

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF = torch.bfloat16
D = ap.D


def _const(value):
    return torch.full((D,), value, dtype=BF, device=DEV)


def _rope_table():
    from cadence_rag_amd.encoder.qwen3 import Qwen3Config, Qwen3Encoder
    return Qwen3Encoder._rope_table(Qwen3Config(max_length=64)).to(DEV)


def _bits(x):
    return x.view(torch.int16)


def _run_tiled(lay, qkv_cpu, hq, hkv, fused):
    """V^T, then crag_enc_attention (or _prefixed when the layout has parents): bf16 [T, hq, 128] on the CPU.
    fused: V^T comes from crag_enc_qk_rope_vt, fed the raw rows (q = s[target], norm weights 4 and 1, every position 0:
    RoPE is the identity) -- its q|k output must be the probe's qkv to the bit, rows past T untouched."""
    from cadence_rag_amd.encoder import ops
    from cadence_rag_amd.encoder.qwen3 import PackedBatch
    t = lay.t
    prefixed = any(p >= 0 for p in lay.parent)
    batch = PackedBatch.build_prefixed(lay.lens, lay.parent, DEV) if prefixed else PackedBatch.build(lay.lens, DEV)
    assert batch.n_tokens == t and batch.cu.cpu().tolist() == lay.cu.tolist()
    qkv = qkv_cpu.to(DEV).contiguous()
    vt = torch.empty(hkv, D, batch.t_pad, dtype=BF, device=DEV)
    if fused:
        raw = qkv.clone()
        raw[:t, : hq * D] = (qkv[:t, : hq * D].float() / ap.Q_GAIN).to(BF)
        ops.qk_rope_vt(raw, _const(ap.Q_GAIN), _const(1.0), _rope_table(), torch.zeros(t, dtype=torch.int32, device=DEV),
                       hq, hkv, ap.EPS, vt, batch.tok_of_pad)
        assert torch.equal(_bits(raw), _bits(qkv))
        qkv = raw
    else:
        ops.v_transpose(qkv, vt, batch.tok_of_pad, hq, hkv)
    out = torch.full((t, hq * D), float("nan"), dtype=BF, device=DEV)
    if prefixed:
        ops.attention_prefixed(qkv, vt, out, batch.cu, batch.cu_pad, batch.blk_seq, batch.blk_q0, batch.parent, hq, hkv, ap.SCALE)
    else:
        ops.attention(qkv, vt, out, batch.cu, batch.cu_pad, batch.blk_seq, batch.blk_q0, hq, hkv, ap.SCALE)
    torch.cuda.synchronize()
    return out.cpu().view(t, hq, D)


def _assert_selected(got, v, tgt, names, grp):
    """got [T, hq, 128] bf16 == V[target] to the bit; a failure names (row, head, target, map)."""
    idx = torch.from_numpy(tgt)
    want = torch.stack([v[idx[:, h], h // grp] for h in range(got.shape[1])], dim=1)
    got = got.float()
    if not torch.equal(got, want):
        bad = torch.nonzero((got != want).any(-1) | torch.isnan(got).any(-1))
        first = [(int(r), int(h), int(tgt[r, h]), names[h]) for r, h in bad[:12].tolist()]
        raise AssertionError(f"{len(bad)} (row, head) outputs are not V[target]; first (row, head, target, map): {first}")


def _assert_mixture(got, ref, names):
    got = got.float()
    assert torch.isfinite(got).all(), torch.nonzero(~torch.isfinite(got).all(-1))[:12].tolist()
    if not torch.allclose(got, ref, atol=ap.ATOL, rtol=ap.RTOL):
        bad = torch.nonzero(((got - ref).abs() > ap.ATOL + ap.RTOL * ref.abs()).any(-1))
        first = [(int(r), int(h), names[h]) for r, h in bad[:12].tolist()]
        raise AssertionError(f"{len(bad)} (row, head) outputs miss the reference, max |d| = "
                             f"{float((got - ref).abs().max()):.3f}; first (row, head, lure): {first}")


def _select_tiled(lens, parent, hq, hkv, maps, seed):
    for n, (lay, names, tgt, qkv) in enumerate(ap.launches(lens, parent, hq, hkv, maps, seed, lure=False)):
        q, k, v = ap.split(qkv, hq, hkv, lay.t)
        assert float(ap.selection_mass(q, k, v, lay.allowed, tgt).max()) <= ap.SELECTION_MASS
        _assert_selected(_run_tiled(lay, qkv, hq, hkv, fused=n % 2 == 1), v, tgt, names, hq // hkv)


def _lure_tiled(lens, parent, hq, hkv, maps, seed):
    for n, (lay, names, forb, qkv) in enumerate(ap.launches(lens, parent, hq, hkv, maps, seed, lure=True)):
        q, k, v = ap.split(qkv, hq, hkv, lay.t)
        ref = ap.reference(q, k, v, lay.allowed)
        assert ap.lure_guard(q, k, v, lay.allowed, forb, ref).all()
        _assert_mixture(_run_tiled(lay, qkv, hq, hkv, fused=n % 2 == 1), ref, names)


def _single(monkeypatch, case):
    if case.single:
        monkeypatch.setenv("CRAG_ATTN_SINGLE", "1")       # read by the launcher on every call
    else:
        monkeypatch.delenv("CRAG_ATTN_SINGLE", raising=False)


@pytest.mark.parametrize("case", ap.ATTENTION_SELECT, ids=lambda c: c.name)
def test_attention_selects_the_one_key(gpu, monkeypatch, case):
    _single(monkeypatch, case)
    _select_tiled(case.lens, None, case.hq, case.hkv, ap.PLAIN_MAPS, case.seed)


@pytest.mark.parametrize("case", ap.ATTENTION_LURE, ids=lambda c: c.name)
def test_attention_ignores_a_forbidden_key_that_would_win(gpu, monkeypatch, case):
    _single(monkeypatch, case)
    _lure_tiled(case.lens, None, case.hq, case.hkv, ap.PLAIN_LURES, case.seed)


@pytest.mark.parametrize("case", ap.PREFIXED, ids=lambda c: c.name)
def test_attention_prefixed_selects_the_one_key(gpu, case):
    _select_tiled(case.lens, case.parent, case.hq, case.hkv, ap.PREFIXED_SELECT_MAPS, case.seed)


@pytest.mark.parametrize("case", ap.PREFIXED, ids=lambda c: c.name)
def test_attention_prefixed_ignores_a_forbidden_key_that_would_win(gpu, case):
    _lure_tiled(case.lens, case.parent, case.hq, case.hkv, ap.PREFIXED_LURES, case.seed + 1)


# ----------------------------------------------------------------------------------------------------------------------
# the fused kernels of <= 32 tokens: q/k-norm and RoPE happen inside, the probes go in raw
# ----------------------------------------------------------------------------------------------------------------------
def _run_small(entry, lay, qkv_cpu, gains):
    from cadence_rag_amd.encoder import ops
    from cadence_rag_amd.encoder.qwen3 import PackedBatch
    hq, hkv = ap.SMALL_HEADS
    t = lay.t
    batch = PackedBatch.build(lay.lens, DEV)
    assert batch.positions.cpu().tolist() == lay.local.tolist()
    qkv = qkv_cpu.to(DEV).contiguous()
    before = qkv.clone()
    qw, kw, table = _const(gains[0]), _const(gains[1]), _rope_table()
    out = torch.full((t + 1, hq * D), 9.0, dtype=BF, device=DEV)
    if entry == "one_block":
        ops.small_attention(qkv[:t], qw, kw, table, batch.positions, out[:t], hq, hkv, ap.EPS, ap.SCALE)
    elif entry == "seqs":
        ops.small_attention_seqs(qkv[:t], qw, kw, table, batch.positions, batch.cu, len(lay.lens), batch.max_len, out[:t],
                                 hq, hkv, ap.EPS, ap.SCALE)
    else:
        # the projection as two split-K partial tiles whose fp32 sums round back to the probe's bf16 values
        g = torch.Generator().manual_seed(t)
        m_pad = (t + 31) // 32 * 32
        a = (torch.randn(t, qkv.shape[1], generator=g) * 0.5).to(DEV)
        parts = torch.zeros(2, m_pad, qkv.shape[1], dtype=torch.float32, device=DEV)
        parts[0, :t], parts[1, :t] = a, qkv[:t].float() - a
        rounded = (parts[0, :t] + parts[1, :t]).to(BF)
        assert torch.equal(rounded, qkv[:t])
        ops.small_attention_seqs_parts(parts, 2, m_pad, qw, kw, table, batch.positions, batch.cu, len(lay.lens),
                                       batch.max_len, out[:t], hq, hkv, ap.EPS, ap.SCALE)
        direct = torch.full_like(out, 9.0)
        ops.small_attention_seqs(rounded, qw, kw, table, batch.positions, batch.cu, len(lay.lens), batch.max_len, direct[:t],
                                 hq, hkv, ap.EPS, ap.SCALE)
        assert torch.equal(_bits(out), _bits(direct))                 # the parts form: the direct form bit for bit
    torch.cuda.synchronize()
    assert torch.equal(_bits(qkv), _bits(before)) and torch.all(out[t] == 9.0)
    return out[:t].cpu().view(t, hq, D)


def _small_select(entry, lens):
    hq, hkv = ap.SMALL_HEADS
    lay, tgt, qkv, gains = ap.small_inputs(lens, lure=False)
    q, k, v = ap.small_qkv_ref(lay, qkv, gains)
    assert float(ap.selection_mass(q, k, v, lay.allowed, tgt).max()) <= ap.SMALL_SELECTION_MASS
    _assert_selected(_run_small(entry, lay, qkv, gains), v, tgt, ap.head_maps(ap.SMALL_MAPS, hq)[0], hq // hkv)


def _small_lure(entry, lens):
    lay, forb, qkv, gains = ap.small_inputs(lens, lure=True)
    q, k, v = ap.small_qkv_ref(lay, qkv, gains)
    ref = ap.reference(q, k, v, lay.allowed)
    assert ap.lure_guard(q, k, v, lay.allowed, forb, ref).all()
    _assert_mixture(_run_small(entry, lay, qkv, gains), ref, ap.head_maps(ap.SMALL_LURES, ap.SMALL_HEADS[0])[0])


ONE_BLOCK = [lens for lens in ap.SMALL_LENS if sum(lens) <= 32]


@pytest.mark.parametrize("lens", ONE_BLOCK, ids=ap.small_id)
def test_small_attention_selects_the_one_key(gpu, lens):
    _small_select("one_block", lens)


@pytest.mark.parametrize("lens", ap.SMALL_LENS, ids=ap.small_id)
def test_small_attention_seqs_selects_the_one_key(gpu, lens):
    _small_select("seqs", lens)


@pytest.mark.parametrize("lens", ap.SMALL_LENS, ids=ap.small_id)
def test_small_attention_seqs_parts_selects_the_one_key(gpu, lens):
    _small_select("parts", lens)


@pytest.mark.parametrize("lens", [lens for lens in ap.SMALL_LURE_LENS if sum(lens) <= 32], ids=ap.small_id)
def test_small_attention_ignores_a_forbidden_key_that_would_win(gpu, lens):
    """One block holds several sequences here: the previous sequence's last key and the next one's first are rows of it."""
    _small_lure("one_block", lens)


@pytest.mark.parametrize("lens", ap.SMALL_LURE_LENS, ids=ap.small_id)
def test_small_attention_seqs_ignores_a_forbidden_key_that_would_win(gpu, lens):
    _small_lure("seqs", lens)


@pytest.mark.parametrize("lens", ap.SMALL_LURE_LENS, ids=ap.small_id)
def test_small_attention_seqs_parts_ignores_a_forbidden_key_that_would_win(gpu, lens):
    _small_lure("parts", lens)
