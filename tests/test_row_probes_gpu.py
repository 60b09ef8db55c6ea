"""Exact probes and bf16-chain checks through the encoder's row operators and its two heads (inputs, references and
case lists: tests/row_probes.py; what the comparisons rest on is proven by tests/test_row_probes_host.py).

Exact probes compare bits.  Chain checks ask rp.MAX_ULPS = 2 bf16 steps for every element and at most rp.MAX_SHARE = 1 %
of the elements with other bits than the fp64 chain reference; every measured share is printed (and appended to the file
CRAG_ROW_PROBE_SHARES names, when set: profiles/row_probes_shares.jsonl is such a run).

Kernels reached: embed_gather_kernel, rmsnorm_kernel, qk_norm_rope_kernel, qk_rope_vt_kernel, kv_append_row through
crag_enc_decode_attention and crag_enc_extend_attention, swiglu_kernel, pool_normalize_kernel (both modes, cu and row
list), lm_head_kernel + lm_argmax_kernel, rerank_head_kernel."""
from __future__ import annotations

import json
import math
import os

import pytest
import torch

import gemm_probes as gp
import row_probes as rp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF = torch.bfloat16
NAN = float("nan")
MARK = 7.0


def _ops():
    from cadence_rag_amd.encoder import ops
    return ops


def _same(got, want):
    """Equal bits, NaN matching NaN (bf16, fp32 or integers)."""
    if got.dtype == BF:
        return rp.same_bits(got, want)
    if got.dtype == torch.float32:
        return (got.contiguous().view(torch.int32) == want.contiguous().view(torch.int32)) | ((got != got) & (want != want))
    return got == want


class Tally:
    """Comparisons stay on the device until check(): one synchronisation per group of launches."""

    def __init__(self):
        self.items = []

    def add(self, label, ok):
        self.items.append((label, ok.all() if ok.dim() else ok))

    def same(self, label, got, want):
        assert got.shape == want.shape and got.dtype == want.dtype, label
        self.add(label, _same(got, want))

    def check(self):
        if not self.items:
            return
        flags = torch.stack([ok for _, ok in self.items]).cpu().tolist()
        bad = [label for (label, _), ok in zip(self.items, flags) if not ok]
        self.items = []
        assert not bad, f"{len(bad)} comparisons failed; first: {bad[:8]}"


def _record(op, shape, share, cap=rp.MAX_SHARE, **extra):
    line = json.dumps({"op": op, "shape": shape, "differing_bit_share": share, "cap": cap, **extra})
    print("row_probe_share", line)
    path = os.environ.get("CRAG_ROW_PROBE_SHARES")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _chain(op, shape, got, want):
    """check_chain under the conditions of the module, the measured share printed first."""
    worst, differ, n = rp.chain_stats(got, want).tolist()
    _record(op, shape, differ / n, max_ulps=worst)
    return rp.check_chain(got, want, rp.MAX_ULPS, rp.MAX_SHARE, f"{op} {shape}")


def _marked(rows, width, dtype=BF, value=MARK):
    return torch.full((rows, width), value, dtype=dtype, device=DEV)


# ----------------------------------------------------------------------------------------------------------------------
# embedding gather
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tokens", rp.EMBED_TOKENS)
@pytest.mark.parametrize("hidden", rp.EMBED_HIDDEN)
def test_embed_gather_copies_the_rows_and_clamps_the_ids(gpu, hidden, n_tokens):
    """Distinct bit patterns; ids 0, vocab - 1, repeats, negative ids (row 0) and ids >= vocab (the last row)."""
    tally = Tally()
    table, id_lists = rp.embed_case(hidden, n_tokens)
    table_d = table.to(DEV)
    for ids in id_lists:
        out = _marked(n_tokens + 1, hidden)
        _ops().embed_gather(ids.to(DEV), table_d, out[:n_tokens])
        tally.same(f"ids {ids[:10].tolist()}", out[:n_tokens], table_d[rp.embed_rows(ids).to(DEV)])
        tally.add("row behind n_tokens", out[n_tokens] == MARK)
    tally.check()


# ----------------------------------------------------------------------------------------------------------------------
# RMSNorm
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", rp.HIDDEN_EDGES)
def test_rmsnorm_exact_probes(gpu, hidden):
    """14 sign-signature rows of +-C: out = +-w bit for bit; with a residual (x = +-C/4, residual_in = +-3C/4) also
    residual_out = +-C; the rows behind `rows` keep their mark."""
    tally = Tally()
    for c in rp.PROBE_C:
        for residual in (False, True):
            p = {k: v.to(DEV) for k, v in rp.rmsnorm_probe(hidden, c, residual).items()}
            out, res_out = _marked(rp.N_SIGNS + 1, hidden), _marked(rp.N_SIGNS + 1, hidden)
            _ops().rmsnorm(p["x"], p["w"], out[:rp.N_SIGNS], rp.EPS, residual_in=p.get("res_in"),
                           residual_out=res_out[:rp.N_SIGNS] if residual else None)
            label = f"C={c} residual={residual}"
            tally.same(label + " out", out[:rp.N_SIGNS], p["want_out"])
            tally.add(label + " out mark", out[rp.N_SIGNS] == MARK)
            if residual:
                tally.same(label + " residual_out", res_out[:rp.N_SIGNS], p["want_res"])
                tally.add(label + " residual_out mark", res_out[rp.N_SIGNS] == MARK)
    tally.check()


@pytest.mark.parametrize("hidden", rp.HIDDEN_EDGES)
def test_rmsnorm_row_does_not_depend_on_its_neighbours(gpu, hidden):
    """The same row gives the same bits alone and as row 12 of 33."""
    g = torch.Generator().manual_seed(hidden)
    block = torch.randn(33, hidden, generator=g).to(BF).to(DEV)
    res = torch.randn(33, hidden, generator=g).to(BF).to(DEV)
    w = (1 + 0.1 * torch.randn(hidden, generator=g)).to(BF).to(DEV)
    tally = Tally()
    for r_in in (None, res):
        many, many_res = _marked(33, hidden), _marked(33, hidden)
        one, one_res = _marked(1, hidden), _marked(1, hidden)
        _ops().rmsnorm(block, w, many, rp.EPS, residual_in=r_in, residual_out=None if r_in is None else many_res)
        _ops().rmsnorm(block[12:13].contiguous(), w, one, rp.EPS, residual_in=None if r_in is None else r_in[12:13].contiguous(),
                       residual_out=None if r_in is None else one_res)
        tally.same("row 12", many[12:13], one)
        tally.same("residual row 12", many_res[12:13], one_res)
    tally.check()


@pytest.mark.parametrize("hidden", rp.CHAIN_HIDDEN)
def test_rmsnorm_follows_the_bf16_chain(gpu, hidden):
    """Random rows at scales 3, 1 and 2e-3 (where eps decides every bit), with and without a residual, against the fp64
    chain: the residual sum is the chain's to the bit, the output within 2 steps and 1 % of the bits."""
    for label, x, w, res in rp.rmsnorm_chain_cases():
        if f"hidden={hidden} " not in label:
            continue
        want, want_res = rp.rmsnorm_ref(x, w, rp.EPS, res)
        out, res_out = _marked(x.shape[0], hidden), _marked(x.shape[0], hidden)
        _ops().rmsnorm(x.to(DEV), w.to(DEV), out, rp.EPS, residual_in=None if res is None else res.to(DEV),
                       residual_out=None if res is None else res_out)
        _chain("rmsnorm", label.split(" ", 1)[1], out, want.to(DEV))
        if res is not None:
            assert bool(_same(res_out, want_res.to(DEV)).all()), label


# ----------------------------------------------------------------------------------------------------------------------
# q/k norm + RoPE: three paths to norm_rope_chunk
# ----------------------------------------------------------------------------------------------------------------------
def _rope_inputs(p):
    """(qkv [T + 1, width] with a NaN row behind the tokens, q_w, k_w, table, positions) on the device."""
    qkv = torch.cat([p.qkv, torch.full((1, p.qkv.shape[1]), NAN, dtype=BF)]).to(DEV)
    return qkv, p.q_w.to(DEV), p.k_w.to(DEV), p.table.to(DEV), p.positions.to(DEV)


def _check_rope_rows(tally, label, p, qkv):
    qk = (p.hq + p.hkv) * 128
    tally.same(label + " q|k", qkv[:p.n_tokens, :qk], p.want.to(DEV))
    tally.same(label + " v untouched", qkv[:p.n_tokens, qk:], p.v.to(DEV))
    tally.add(label + " row behind n_tokens", torch.isnan(qkv[p.n_tokens]))


@pytest.mark.parametrize("hq,hkv", rp.ROPE_HEADS)
def test_qk_norm_rope_exact_probes(gpu, hq, hkv):
    """+-C head vectors under distinct q / k weight patterns and the probe tables (identity, quarter turn, position and
    column in the cos and in the sin slot, a cos that is no bf16 value), 1 and 5 tokens at positions out of order:
    the q|k columns equal the expectation bit for bit, the v columns and the row behind n_tokens are untouched."""
    tally = Tally()
    for p in rp.rope_probes(heads=((hq, hkv),)):
        qkv, q_w, k_w, table, pos = _rope_inputs(p)
        _ops().qk_norm_rope(qkv, q_w, k_w, table, pos, hq, hkv, rp.EPS)
        _check_rope_rows(tally, f"tokens={p.n_tokens} table={p.kind}", p, qkv)
    tally.check()


@pytest.mark.parametrize("hq,hkv", rp.ROPE_HEADS)
def test_qk_rope_vt_exact_probes(gpu, hq, hkv):
    """The same probes through the launch that also transposes V (its V^T is pinned elsewhere): q|k match."""
    tally = Tally()
    for p in rp.rope_probes(heads=((hq, hkv),)):
        qkv, q_w, k_w, table, pos = _rope_inputs(p)
        tok_of_pad = torch.full((32,), -1, dtype=torch.int32)
        tok_of_pad[:p.n_tokens] = torch.arange(p.n_tokens, dtype=torch.int32)
        vt = torch.empty(hkv, 128, 32, dtype=BF, device=DEV)
        _ops().qk_rope_vt(qkv, q_w, k_w, table, pos, hq, hkv, rp.EPS, vt, tok_of_pad.to(DEV))
        _check_rope_rows(tally, f"tokens={p.n_tokens} table={p.kind}", p, qkv)
    tally.check()


def _append_case(p, seqs):
    """A one-layer KvCache of 8 slots x APPEND_MAX_LEN rows, NaN everywhere but the rows a slot already holds (0.5)."""
    from cadence_rag_amd.encoder.generate import KvCache
    cache = KvCache(1, 8, p.hkv, rp.APPEND_MAX_LEN, DEV)
    cache.k.fill_(NAN)
    cache.v.fill_(NAN)
    for slot, m, _ in seqs:
        cache.k[0, slot, :, :m] = 0.5
        cache.v[0, slot, :, :m] = 0.5
        cache.lens[slot] = m
    return cache


def _check_append(tally, label, p, seqs, cache, before_k, before_v):
    """The appended k rows are the probe's expectation and the v rows the raw projections, read back through
    KvCache.keys / values; every other row of the cache keeps its bits."""
    hq, hkv = p.hq, p.hkv
    want_k = p.want[:, hq * 128:].view(p.n_tokens, hkv, 128).to(DEV)
    want_v = p.v.view(p.n_tokens, hkv, 128).to(DEV)
    row = 0
    for slot, m, n in seqs:
        cache.lens[slot] = m + n
        tally.same(f"{label} slot {slot} k rows", cache.keys(0, slot)[m:].contiguous(), want_k[row:row + n])
        tally.same(f"{label} slot {slot} v rows", cache.values(0, slot)[m:].contiguous(), want_v[row:row + n])
        before_k[0, slot, :, m:m + n] = want_k[row:row + n].transpose(0, 1)
        before_v[0, slot, :, m:m + n] = want_v[row:row + n].transpose(0, 1)
        row += n
    tally.same(label + " whole k cache", cache.k, before_k)
    tally.same(label + " whole v cache", cache.v, before_v)


@pytest.mark.parametrize("hq,hkv", rp.APPEND_HEADS)
def test_decode_appends_the_probe_rows_to_the_cache(gpu, hq, hkv):
    """kv_append_row under crag_enc_decode_attention against an expectation that comes from no kernel: the k row at
    position len of the slot is rope_rotate(+-k_w), the v row the raw projection.  (The entry takes hq / hkv of 2 or 4:
    three of the five head counts.)"""
    ops, tally = _ops(), Tally()
    for p in rp.rope_probes(heads=((hq, hkv),), positions=rp.append_positions(rp.DECODE_SEQS)):
        seqs = rp.DECODE_SEQS[p.n_tokens]
        cache = _append_case(p, seqs)
        before_k, before_v = cache.k.clone(), cache.v.clone()
        kc, vc = cache.layer(0)
        out = torch.empty(p.n_tokens, hq * 128, dtype=BF, device=DEV)
        ops.decode_attention(p.qkv.to(DEV), p.q_w.to(DEV), p.k_w.to(DEV), p.table.to(DEV), kc, vc, [s for s, _, _ in seqs],
                             [m for _, m, _ in seqs], out, hq, hkv, rp.EPS, 1.0 / math.sqrt(128),
                             ops.decode_workspace(8, hq, rp.APPEND_MAX_LEN, DEV))
        _check_append(tally, f"tokens={p.n_tokens} table={p.kind}", p, seqs, cache, before_k, before_v)
    tally.check()


@pytest.mark.parametrize("hq,hkv", rp.APPEND_HEADS)
def test_extend_appends_the_probe_rows_to_the_cache(gpu, hq, hkv):
    """The same through crag_enc_extend_attention: 3 + 2 new rows at positions 13, 14, 15 and 0, 1, and one row at 15."""
    ops, tally = _ops(), Tally()
    for p in rp.rope_probes(heads=((hq, hkv),), positions=rp.append_positions(rp.EXTEND_SEQS)):
        seqs = rp.EXTEND_SEQS[p.n_tokens]
        cache = _append_case(p, seqs)
        before_k, before_v = cache.k.clone(), cache.v.clone()
        kc, vc = cache.layer(0)
        out = torch.empty(p.n_tokens, hq * 128, dtype=BF, device=DEV)
        ops.extend_attention(p.qkv.to(DEV), p.q_w.to(DEV), p.k_w.to(DEV), p.table.to(DEV), kc, vc, [s for s, _, _ in seqs],
                             [m for _, m, _ in seqs], [n for _, _, n in seqs], out, hq, hkv, rp.EPS, 1.0 / math.sqrt(128),
                             ops.extend_workspace(8, hq, p.n_tokens, rp.APPEND_MAX_LEN, DEV))
        _check_append(tally, f"tokens={p.n_tokens} table={p.kind}", p, seqs, cache, before_k, before_v)
    tally.check()


@pytest.mark.parametrize("hq,hkv", rp.ROPE_HEADS)
def test_qk_norm_rope_follows_the_bf16_chain(gpu, hq, hkv):
    """Random head vectors under the real RoPE table against the fp64 chain (norm output rounded, weighted element
    rounded, table cast to bf16, one rounding of n cos + rotate_half(n) sin)."""
    heads, v, q_w, k_w, table, pos = rp.rope_chain_case(hq, hkv)
    want = rp.norm_rope_ref(heads, rp.head_weights(q_w, k_w, hq, hkv), table, pos, rp.EPS).view(heads.shape[0], -1)
    qkv = torch.cat([heads.view(heads.shape[0], -1), v], dim=1).to(DEV)
    _ops().qk_norm_rope(qkv, q_w.to(DEV), k_w.to(DEV), table.to(DEV), pos.to(DEV), hq, hkv, rp.EPS)
    qk = (hq + hkv) * 128
    _chain("qk_norm_rope", f"hq={hq} hkv={hkv} tokens={heads.shape[0]}", qkv[:, :qk].contiguous(), want.to(DEV))
    assert bool(_same(qkv[:, qk:].contiguous(), v.to(DEV)).all())


# ----------------------------------------------------------------------------------------------------------------------
# SwiGLU
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up", rp.SWIGLU_UPS)
def test_swiglu_over_every_gate(gpu, up):
    """All 65 536 gate patterns against one up value: NaN exactly where fp64 gives NaN (NaN gates and -inf); every other
    output a member of the admissible set (the two bf16 neighbours of the fp64 silu, times up) -- where the gate or its
    silu lies below the normal numbers a zero of the product's sign is accepted as well; over the gates whose silu is a
    normal number at most 1 % differ from the member of the correctly rounded silu.

    Below the normals the kernel (MI355X) keeps the denormals: of the 16 070 gates whose silu or who themselves lie
    there, every output is a member of the set and none needed the zero ("small_as_zero": 0 of "small" in
    profiles/row_probes_shares.jsonl).  Before the overflow of exp(-g) was handled in swiglu_kernel the six gates
    -89 .. -91.5 (silu -2e-37 .. -1e-38, normal numbers) came out as -0 and failed this test, and ten more between -92
    and -96.5 were -0 where the set holds a denormal."""
    e = {k: v.to(DEV) for k, v in rp.swiglu_exhaustive(up).items()}
    out = _marked(9, 8192)
    _ops().swiglu(torch.cat([e["gate"], e["up"]], dim=1).contiguous(), out[:8])
    got = out[:8]
    is_nan = torch.isnan(got)
    as_zero = e["small"] & _same(got, e["zero"])
    ok = gp.member(got, e["lo"], e["hi"]) | as_zero
    differ = (~_same(got, e["exact"]) & e["normal"]).sum()
    outside = e["gate"][~e["nan"] & ~ok]
    counts = torch.stack([differ, e["normal"].sum(), (as_zero & ~gp.member(got, e["lo"], e["hi"])).sum(), e["small"].sum(),
                          (is_nan != e["nan"]).sum(), outside.numel() + 0 * differ, (out[8] != MARK).sum()]).tolist()
    share = counts[0] / counts[1]
    _record("swiglu", f"all gates, up={up}", share, small_as_zero=counts[2], small=counts[3])
    assert counts[4] == 0, "NaN where fp64 has a number, or a number where fp64 has NaN"
    assert counts[5] == 0, f"{counts[5]} outputs outside the admissible set; gates: {sorted(set(outside.float().tolist()))[:16]}"
    assert share <= rp.MAX_SHARE
    assert counts[6] == 0


@pytest.mark.parametrize("inter", rp.SWIGLU_INTERS)
def test_swiglu_selection_probes(gpu, inter):
    """Gate 32 (silu exactly 32) against up of distinct patterns: the output is up * 2^5 -- the + inter offset and the
    2 * inter row stride; up 1 against gates of distinct patterns >= 32: the output is the gate.  1 and 3 rows, the row
    behind them untouched."""
    tally = Tally()
    for rows in rp.SWIGLU_ROWS:
        s = {k: v.to(DEV) for k, v in rp.swiglu_selection(inter, rows).items()}
        for name in ("up", "gate"):
            out = _marked(rows + 1, inter)
            _ops().swiglu(s[name + "_in"], out[:rows])
            tally.same(f"rows={rows} {name}", out[:rows], s[name + "_want"])
            tally.add(f"rows={rows} {name} mark", out[rows] == MARK)
    tally.check()


# ----------------------------------------------------------------------------------------------------------------------
# pooling
# ----------------------------------------------------------------------------------------------------------------------
POOL_RTOL = 1e-6     # fp32 round-off of a 256-thread sum of squares, a square root and a division: derived, not measured


def _check_pool(tally, label, out, want64, n):
    """out [n + 1, out_dim] fp32 against want [n, out_dim] fp64: within POOL_RTOL, the signs exact, a zero row exactly
    zero, the row behind untouched."""
    want = want64.to(DEV)
    got = out[:n].double()
    tally.add(label + " value", (got - want).abs() <= POOL_RTOL * want.abs())
    tally.add(label + " sign", (torch.signbit(got) == torch.signbit(want)) | (want == 0))
    tally.add(label + " mark", out[n] == MARK)


@pytest.mark.parametrize("hidden", rp.POOL_HIDDEN)
def test_pool_normalize_last_token_probes(gpu, hidden):
    """Mode 0: every token has its own sign signature, the normed row is exactly +-w, so the output is
    +-w[:out_dim] / ||w[:out_dim]|| with the pooled token's signs -- through cu (lengths 1, 0, 2, 8, 0) and through a row
    list (repeats, 0, the last row), with and without a delta (+-C/4 + +-3C/4); an empty sequence gives a zero row."""
    ops, tally = _ops(), Tally()
    spans = rp.pool_spans()
    cu = torch.tensor(rp.POOL_CU, dtype=torch.int32, device=DEV)
    rows = torch.tensor(rp.POOL_ROWS, dtype=torch.int64, device=DEV)
    for with_delta in (False, True):
        p = rp.pool_probe(hidden, with_delta)
        hs, w = p["hs"].to(DEV), p["w"].to(DEV)
        delta = p["delta"].to(DEV) if with_delta else None
        by_cu = torch.stack([p["normed"][t1 - 1] if t1 > t0 else torch.zeros(hidden, dtype=torch.float64) for t0, t1 in spans])
        by_rows = p["normed"][list(rp.POOL_ROWS)]
        for out_dim in rp.pool_out_dims(hidden):
            label = f"delta={with_delta} out_dim={out_dim}"
            out = _marked(len(spans) + 1, out_dim, torch.float32)
            ops.pool_normalize(hs, w, cu, out[:len(spans)], out_dim, 0, rp.EPS, delta=delta)
            _check_pool(tally, label + " cu", out, rp.pool_want(by_cu, out_dim), len(spans))
            tally.add(label + " empty sequences", out[[1, 4]] == 0)
            out = _marked(len(rp.POOL_ROWS) + 1, out_dim, torch.float32)
            ops.pool_normalize_rows(hs, w, rows, out[:len(rp.POOL_ROWS)], out_dim, rp.EPS, delta=delta)
            _check_pool(tally, label + " rows", out, rp.pool_want(by_rows, out_dim), len(rp.POOL_ROWS))
    tally.check()


@pytest.mark.parametrize("hidden", rp.POOL_HIDDEN)
def test_pool_normalize_mean_probes(gpu, hidden):
    """Mode 1: integer-valued tokens in sequences of 1, 2 and 8, so the mean is exact; empty sequences give zero rows."""
    ops, tally = _ops(), Tally()
    spans = rp.pool_spans()
    cu = torch.tensor(rp.POOL_CU, dtype=torch.int32, device=DEV)
    toks = rp.pool_mean_tokens(hidden)
    mean = rp.pooled_row_ref(toks, None, spans, 1, rp.EPS)
    for out_dim in rp.pool_out_dims(hidden):
        out = _marked(len(spans) + 1, out_dim, torch.float32)
        ops.pool_normalize(toks.to(DEV), None, cu, out[:len(spans)], out_dim, 1, rp.EPS)
        _check_pool(tally, f"out_dim={out_dim}", out, rp.pool_want(mean, out_dim), len(spans))
        tally.add(f"out_dim={out_dim} empty sequences", out[[1, 4]] == 0)
    tally.check()


@pytest.mark.parametrize("hidden", rp.CHAIN_HIDDEN)
def test_pooled_row_follows_the_bf16_chain(gpu, hidden):
    """Random rows + delta through the row list at out_dim = hidden: the fp32 output times the reference row's norm,
    rounded to bf16, is the normed row again -- within 2 steps and 1 % of the bits of the fp64 chain."""
    hs, delta, w = rp.pool_chain_case(hidden)
    want = rp.to_bf16(rp.pooled_row_ref(hs, w, [(t, t + 1) for t in range(rp.N_SIGNS)], 0, rp.EPS, delta))
    out = torch.empty(rp.N_SIGNS, hidden, dtype=torch.float32, device=DEV)
    _ops().pool_normalize_rows(hs.to(DEV), w.to(DEV), torch.arange(rp.N_SIGNS, device=DEV), out, hidden, rp.EPS, delta=delta.to(DEV))
    back = rp.to_bf16(out.cpu().double() * want.double().norm(dim=1, keepdim=True))
    _chain("pool_normalize", f"hidden={hidden} rows={rp.N_SIGNS} delta=1", back, want)


# ----------------------------------------------------------------------------------------------------------------------
# lm_head + argmax
# ----------------------------------------------------------------------------------------------------------------------
def _lm_head(tally, label, hs, w, lm, want_logits, want_tokens, delta=None, banned=None):
    """One crag_enc_lm_head call over the rows of hs: logits and tokens to the bit, the row behind n_rows untouched."""
    n, vocab = hs.shape[0], lm.shape[0]
    logits = _marked(n + 1, vocab, torch.float32)
    token = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
    ban = None if not banned else torch.tensor(banned, dtype=torch.int32, device=DEV)
    _ops().lm_head(hs.to(DEV), w.to(DEV), lm.to(DEV), logits[:n], token[:n], rp.EPS,
                   delta=None if delta is None else delta.to(DEV), banned=ban)
    tally.same(label + " logits", logits[:n], want_logits.float().to(DEV))
    tally.add(label + " logits mark", logits[n] == MARK)
    tally.same(label + " token", token[:n], torch.tensor(want_tokens, dtype=torch.int32, device=DEV))
    tally.add(label + " token mark", token[n] == -7)


@pytest.mark.parametrize("n_rows", rp.LM_ROWS)
@pytest.mark.parametrize("hidden", rp.LM_HIDDEN)
def test_lm_head_integer_probes(gpu, hidden, n_rows):
    """+-C rows under weights in {+-1, +-2} against lm of integers in -3..3: every logit is an integer below 2^24, so the
    fp32 output equals the int64 matmul whatever the MFMA order.  hidden 64 and 192 run the 64-wide tail loop alone, 256
    the main loop alone, 320 and 2624 both; every vocabulary around the 16-row tile and the 256-row workgroup; with and
    without a delta; the greedy token is the lowest id among the maxima (ties are common here)."""
    tally = Tally()
    for with_delta in (False, True):
        p = rp.int_rows(n_rows, hidden, with_delta, f"lm{n_rows}")
        for vocab in rp.LM_VOCAB:
            lm, want = rp.lm_integer(p, vocab)
            _lm_head(tally, f"delta={with_delta} vocab={vocab}", p["hs"], p["w"], lm, want, rp.argmax_ref(want.double()), p["delta"])
        tally.check()


@pytest.mark.parametrize("n_rows", rp.LM_ROWS)
@pytest.mark.parametrize("hidden", rp.LM_HIDDEN)
def test_lm_head_one_hot_probes(gpu, hidden, n_rows):
    """lm[v] = e_k(v) under w of distinct patterns: logits[r][v] = float(+-w[k(v)]) bit for bit; vocab = hidden + 1 walks
    every k, the small vocabularies the tile edges."""
    tally = Tally()
    for vocab in rp.LM_VOCAB + (hidden + 1,):
        hs, w, lm, want = rp.lm_one_hot(hidden, n_rows, vocab)
        _lm_head(tally, f"vocab={vocab}", hs, w, lm, want, rp.argmax_ref(want.double()))
    tally.check()


def test_lm_argmax_cases(gpu):
    """Planted integer logits through the same entry: an all-NaN row and a row with every finite id banned give -1; a
    row of -inf with one finite value; the maximum at id 0 and at the last id; ties at vocabularies of 1023, 1024 and
    1025 (one id per thread, then a second trip), with and without the lower id banned."""
    tally = Tally()
    for c in rp.argmax_cases():
        logits = rp.head_ref(c["hs"], c["w"], rp.EPS, c["lm"])[1]
        _lm_head(tally, c["name"], c["hs"], c["w"], c["lm"], logits, rp.argmax_ref(logits, c["banned"]), banned=c["banned"])
    tally.check()


# ----------------------------------------------------------------------------------------------------------------------
# rerank head
# ----------------------------------------------------------------------------------------------------------------------
SCORE_RTOL = 1e-6    # expf, one addition and one division in fp32; below the normal numbers the fp32 score is 0 or denormal


@pytest.mark.parametrize("hidden", rp.RERANK_HIDDEN)
def test_rerank_head_integer_probes(gpu, hidden):
    """The integer setup over a row list with repeats: logit_yes and logit_no are the exact integers; the score is the
    fp64 value within 1e-6, exactly 0.5 at yes == no, exactly 1.0 at yes - no = 200, and at yes - no = -200 finite,
    >= 0 and below the normal numbers (the form that cannot overflow)."""
    ops, tally = _ops(), Tally()
    rows = torch.tensor(rp.RERANK_ROWS, dtype=torch.int64)
    n = rows.numel()
    for with_delta in (False, True):
        p = rp.int_rows(8, hidden, with_delta, "rerank")
        for kind in rp.RERANK_KINDS:
            lm = rp.rerank_lm(p, kind)
            want = (p["normed"][rows] @ lm.long().t()).double()                       # [n, 2]: yes, no
            score = rp.score_ref(want[:, 0], want[:, 1]).to(DEV)
            out = _marked(n + 1, 3, torch.float32)
            ops.rerank_head(p["hs"].to(DEV), p["w"].to(DEV), rows.to(DEV), lm.to(DEV), out[:n], rp.EPS,
                            delta=None if p["delta"] is None else p["delta"].to(DEV))
            label = f"delta={with_delta} {kind}"
            tally.same(label + " logits", out[:n, :2].contiguous(), want.float().to(DEV))
            got = out[:n, 2].double()
            tally.add(label + " score", (got - score).abs() <= SCORE_RTOL * score + rp.TINY)
            tally.add(label + " mark", out[n] == MARK)
            last = (rows == 7).to(DEV)                                                # the all-positive row: yes - no = +-200
            if kind == "equal":
                tally.add(label + " exactly one half", out[:n, 2] == 0.5)
            elif kind == "plus200":
                tally.add(label + " exactly one", out[:n, 2][last] == 1.0)
            elif kind == "minus200":
                tiny = out[:n, 2][last]
                tally.add(label + " zero or denormal", torch.isfinite(tiny) & (tiny >= 0) & (tiny < rp.TINY))
        tally.check()
