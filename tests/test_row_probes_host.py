"""What tests/test_row_probes_gpu.py rests on, proven without a GPU (tests/row_probes.py):

  * on every random chain input the GPU file uses, an fp32 chain -- also with its reciprocal square root scaled by
    1 +- 4 * 2^-23 -- stays within 2 bf16 steps of the fp64 chain reference and under a TENTH of the share cap; the same
    for silu with exp replaced by exp2(float32(x * log2 e)): the conditions leave a real kernel ten times the room a
    correct one needs;
  * every exact probe's expected tensor equals the fp64 chain reference of the same input bit for bit, also under the
    perturbed reciprocal root;
  * chains altered on purpose fail check_chain on the same inputs: an inner rounding dropped, the table not cast, eps
    1e-5 on the small-magnitude rows, q weights used for k heads, the partner of the wrong sign."""
from __future__ import annotations

import math

import pytest
import torch

import gemm_probes as gp
import row_probes as rp

BF, F32, F64 = rp.BF, rp.F32, rp.F64
SCALES = rp.RSTD_SCALES
TENTH = rp.MAX_SHARE / 10


# ----------------------------------------------------------------------------------------------------------------------
# the helpers themselves
# ----------------------------------------------------------------------------------------------------------------------
def test_to_bf16_rounds_fp64_once():
    # 1 + 2^-8 + 2^-40 lies above the tie between 1 and 1 + 2^-7: fp32 drops the 2^-40, and the tie then goes to even
    x = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -40, 1 + 2.0 ** -8, -(1 + 2.0 ** -8 + 2.0 ** -40), 0.0, math.inf, 3.0e38], dtype=F64)
    assert x.float().to(BF).tolist()[:2] == [1.0, 1.0]
    assert rp.to_bf16(x).tolist()[:5] == [1 + 2.0 ** -7, 1.0, -(1 + 2.0 ** -7), 0.0, math.inf]
    g = torch.Generator().manual_seed(1)
    y = torch.randn(100000, generator=g, dtype=F64) * torch.tensor(2.0, dtype=F64) ** torch.randint(-40, 40, (100000,), generator=g)
    r = rp.to_bf16(y).double()
    for step in (True, False):
        other = gp._bf16_step(rp.to_bf16(y), up=step).double()
        assert bool(((r - y).abs() <= (other - y).abs()).all())


def test_bf16_ulps_and_check_chain():
    v = torch.tensor([1.0, 1.0, -0.0, 0.0, rp.NAN, rp.NAN, 2.0 ** -133, -1.0], dtype=BF)
    w = torch.tensor([1.0078125, 0.99609375, 0.0, -(2.0 ** -133), rp.NAN, 1.0, -(2.0 ** -133), -1.0078125], dtype=BF)
    assert rp.bf16_ulps(v, w).tolist() == [1, 1, 0, 1, 0, rp.FAR, 2, 1]
    assert rp.same_bits(v, w).tolist() == [False, False, False, False, True, False, False, False]
    a = torch.ones(1000, dtype=BF)
    b = a.clone()
    b[:10] = 1.0078125
    assert rp.check_chain(b, a, 2, 0.01) == 0.01
    b[10] = 1.0078125
    assert rp.fails_chain(b, a, 2, 0.01)                       # the share
    c = a.clone()
    c[0] = 1.0234375                                           # three steps
    assert rp.fails_chain(c, a, 2, 0.01) and not rp.fails_chain(c, a, 3, 0.01)
    c[0] = rp.NAN
    assert rp.fails_chain(c, a, 1000, 0.5)


def test_c_times_rsqrt_rounds_to_one():
    """C * rsqrt(C^2 + eps) in fp32 with the root off by up to 4 ulps either way rounds to exactly 1.0 in bf16."""
    eps = torch.tensor(rp.EPS, dtype=F32)
    for c in (1024.0, 3.0, 0.5) + rp.PROBE_C:
        c32 = torch.tensor(c, dtype=F32)
        for k in range(-4, 5):
            rstd = torch.rsqrt(c32 * c32 + eps) * torch.tensor(1 + k * 2.0 ** -23, dtype=F32)
            assert float((c32 * rstd).to(BF)) == 1.0, (c, k)


# ----------------------------------------------------------------------------------------------------------------------
# RMSNorm
# ----------------------------------------------------------------------------------------------------------------------
def test_rmsnorm_fp32_chains_meet_the_conditions_with_room_and_altered_chains_fail():
    for label, x, w, res in rp.rmsnorm_chain_cases():
        want, want_res = rp.rmsnorm_ref(x, w, rp.EPS, res)
        assert SCALES[1] == 1 + 4 * 2.0 ** -23 and SCALES[2] == 1 - 4 * 2.0 ** -23
        for scale in SCALES:
            got, got_res = rp.rmsnorm_chain(x, w, rp.EPS, res, dtype=F32, rstd_scale=scale)
            assert rp.check_chain(got, want, rp.MAX_ULPS, TENTH, label) <= TENTH
            if res is not None:
                assert torch.equal(rp.bits(got_res), rp.bits(want_res))
        assert rp.fails_chain(rp.rmsnorm_chain(x, w, rp.EPS, res, dtype=F32, inner=False)[0], want), label
        if "scale=0.002" in label:
            assert rp.fails_chain(rp.rmsnorm_chain(x, w, 1e-5, res, dtype=F32)[0], want), label
            assert rp.fails_chain(rp.rmsnorm_chain(x, w, 0.0, res, dtype=F32)[0], want), label
        if res is not None:                                    # the residual sum kept in fp32 instead of bf16
            s = x.float() + res.float()
            unrounded = (w.float() * (s * torch.rsqrt((s * s).mean(-1, keepdim=True) + rp.EPS)).to(BF).float()).to(BF)
            assert rp.fails_chain(unrounded, want), label


@pytest.mark.parametrize("hidden", rp.HIDDEN_EDGES)
def test_rmsnorm_probes_equal_the_chain_reference(hidden):
    for c in rp.PROBE_C:
        for residual in (False, True):
            p = rp.rmsnorm_probe(hidden, c, residual)
            assert len({int(b) for b in rp.bits(p["w"])}) == hidden
            for dtype, scale in [(F64, 1.0)] + [(F32, s) for s in SCALES]:
                out, res = rp.rmsnorm_chain(p["x"], p["w"], rp.EPS, p.get("res_in"), dtype=dtype, rstd_scale=scale)
                assert torch.equal(rp.bits(out), rp.bits(p["want_out"]))
                if residual:
                    assert torch.equal(rp.bits(res), rp.bits(p["want_res"]))
    # every element index has its own signature across the 14 rows
    sg = rp.signs(hidden, range(rp.N_SIGNS))
    assert len({tuple(col) for col in sg.t().tolist()}) == hidden


# ----------------------------------------------------------------------------------------------------------------------
# q/k norm + RoPE
# ----------------------------------------------------------------------------------------------------------------------
def test_rope_probes_equal_the_chain_reference():
    n = 0
    for p in rp.rope_probes():
        for kw in [dict(dtype=F64)] + [dict(dtype=F32, rstd_scale=s) for s in SCALES]:
            assert torch.equal(rp.bits(p.chain(**kw)), rp.bits(p.want)), (p.hq, p.hkv, p.n_tokens, p.kind, kw)
        assert not bool(torch.isnan(p.want.float()).any())
        assert sorted(p.positions.tolist())[-1] == rp.ROPE_MAX_POS - 1 and (p.n_tokens == 1 or 0 in p.positions.tolist())
        n += 1
    assert n == len(rp.ROPE_HEADS) * len(rp.ROPE_TOKENS) * len(rp.ROPE_TABLES)
    assert rp.APPEND_HEADS == ((4, 2), (16, 8), (32, 8))
    assert not set(rp.bits(rp.pattern_weights(128, rp.Q_BASE)).tolist()) & set(rp.bits(rp.pattern_weights(128, rp.K_BASE)).tolist())


def test_rope_probe_expectations_by_hand():
    """The expected tensors against the issue's closed forms, independent of rope_rotate."""
    for p in rp.rope_probes(heads=((20, 4),)):
        n = (p.sign * p.w.double())                                          # [T, heads, 128]: +-w
        want = p.want.view(p.n_tokens, -1, 128).double()
        pos = p.positions.long()
        col = 2.0 ** -(pos % 8).double()[:, None, None] * (1 + (torch.arange(128) % 64).double() / 64)[None, None, :]
        if p.kind in ("identity", "cast", "cast-3"):
            assert torch.equal(want, n)
        elif p.kind == "quarter":
            assert torch.equal(want[..., :64], -n[..., 64:]) and torch.equal(want[..., 64:], n[..., :64])
        elif p.kind == "poscol-cos":
            assert torch.equal(want, p.sign * col)
        else:
            assert torch.equal(want, torch.cat([-p.sign[..., 64:], p.sign[..., :64]], -1) * col)


def test_the_cast_probe_bites_only_with_the_second_value():
    """With cos = 1 + 2^-10 an uncast table rounds back to +-w (the probe pins the result, not the cast); with
    1 + 3 * 2^-10 an uncast table changes bits."""
    for kind, bites in (("cast", False), ("cast-3", True)):
        p = rp.RopeProbe(20, 4, 5, kind)
        uncast = p.chain(dtype=F32, cast_table=False)
        assert (not torch.equal(rp.bits(uncast), rp.bits(p.want))) == bites


@pytest.mark.parametrize("hq,hkv", rp.ROPE_HEADS)
def test_rope_fp32_chains_meet_the_conditions_with_room_and_altered_chains_fail(hq, hkv):
    heads, _, q_w, k_w, table, pos = rp.rope_chain_case(hq, hkv)
    w = rp.head_weights(q_w, k_w, hq, hkv)
    want = rp.norm_rope_ref(heads, w, table, pos, rp.EPS)
    for scale in SCALES:
        got = rp.norm_rope_chain(heads, w, table, pos, rp.EPS, dtype=F32, rstd_scale=scale)
        assert rp.check_chain(got, want, rp.MAX_ULPS, TENTH) <= TENTH
    wrong = {"inner rounding dropped": dict(inner=False), "table not cast": dict(cast_table=False),
             "partner of the wrong sign": dict(wrong_partner=True)}
    for name, kw in wrong.items():
        assert rp.fails_chain(rp.norm_rope_chain(heads, w, table, pos, rp.EPS, dtype=F32, **kw), want), name
    q_for_k = rp.norm_rope_chain(heads, rp.head_weights(q_w, q_w, hq, hkv), table, pos, rp.EPS, dtype=F32)
    assert rp.fails_chain(q_for_k, want)
    wrong_pos = rp.norm_rope_chain(heads, w, table, pos.roll(1), rp.EPS, dtype=F32)
    assert rp.fails_chain(wrong_pos, want)


def test_rope_probes_catch_the_wrong_weights_and_the_wrong_partner():
    for p in rp.rope_probes(heads=((20, 4),)):
        if p.kind in ("identity", "quarter"):
            q_for_k = rp.norm_rope_chain(p.heads, rp.head_weights(p.q_w, p.q_w, p.hq, p.hkv), p.table, p.positions, rp.EPS)
            assert not torch.equal(rp.bits(q_for_k.view(p.n_tokens, -1)), rp.bits(p.want))
        if p.kind in ("quarter", "poscol-sin"):
            assert not torch.equal(rp.bits(p.chain(wrong_partner=True)), rp.bits(p.want))


# ----------------------------------------------------------------------------------------------------------------------
# SwiGLU
# ----------------------------------------------------------------------------------------------------------------------
def _silu_fp32(gate, exp2_form: bool, ulps_off: int = 0):
    x = gate.float()
    if exp2_form:
        e = torch.exp2((-x * torch.tensor(math.log2(math.e), dtype=F32)).float())
    else:
        e = torch.exp(-x)
    s = x / (1.0 + e)
    if ulps_off:
        s = s * torch.tensor(1 + ulps_off * 2.0 ** -23, dtype=F32)
    return s.to(BF)


@pytest.mark.parametrize("up", rp.SWIGLU_UPS)
def test_swiglu_exhaustive_reference(up):
    e = rp.swiglu_exhaustive(up)
    assert int(e["nan"].sum()) == 2 * 127 + 1                              # the NaN patterns of both signs and -inf
    assert bool(gp.member(e["exact"], e["lo"], e["hi"])[~e["nan"]].all())
    assert int(e["normal"].sum()) > 45000 and int(e["small"].sum()) > 256
    for exp2_form in (False, True):
        for off in (0, 8, -8):
            got = (_silu_fp32(e["gate"], exp2_form, off).float() * e["up"].float()).to(BF)
            # an fp32 exp overflows where fp64 does not (gates below -88.7: silu about -1e-37, still a normal number); the
            # CPU stand-in is asked for membership only where it does not
            reach = e["normal"] & (e["gate"].float() > -88.0)
            assert bool(gp.member(got, e["lo"], e["hi"])[reach].all())
            share = float((~rp.same_bits(got, e["exact"]))[reach].float().mean())
            assert share <= 0.4 * rp.MAX_SHARE, (up, exp2_form, off, share)
            if off == 0:
                assert share <= TENTH, (up, exp2_form, share)
    # silu not rounded before the product: over all normal gates 2-3 % of the bits change (above the cap), over
    # 2^-6 < |gate| < 16 a quarter (outside, silu is the gate, half the gate or next to nothing and the rounding is no
    # rounding); up = 1 is no product at all
    g = e["gate"].float()
    differ = ~rp.same_bits((g / (1.0 + torch.exp(-g)) * e["up"].float()).to(BF), e["exact"])
    if up != 1.0:
        assert float(differ[e["normal"]].float().mean()) > 2 * rp.MAX_SHARE
        assert float(differ[e["normal"] & (g.abs() > 2.0 ** -6) & (g.abs() < 16)].float().mean()) > 0.2


@pytest.mark.parametrize("inter", rp.SWIGLU_INTERS)
def test_swiglu_selection_probes_are_exact(inter):
    s = rp.swiglu_selection(inter, 3)
    for name in ("up", "gate"):
        x, want = s[name + "_in"], s[name + "_want"]
        lo, hi = gp.swiglu_set(x[:, :inter], x[:, inter:])          # (silu(g) = g (1 - e^-g) in fp64: just below g)
        g64 = x[:, :inter].double()
        rounded = (rp.to_bf16(g64 / (1.0 + torch.exp(-g64))).float() * x[:, inter:].float()).to(BF)
        assert torch.equal(rp.bits(rounded), rp.bits(want)) and bool(gp.member(want, lo, hi).all())
        assert bool(torch.isfinite(want.float()).all())
        for exp2_form in (False, True):
            got = (_silu_fp32(x[:, :inter], exp2_form).float() * x[:, inter:].float()).to(BF)
            assert torch.equal(rp.bits(got), rp.bits(want))
    assert len({int(b) for b in rp.bits(s["up_want"][0])}) == min(inter, 9728)


# ----------------------------------------------------------------------------------------------------------------------
# embedding gather, pooling
# ----------------------------------------------------------------------------------------------------------------------
def test_embed_case_holds_what_it_promises():
    for hidden in rp.EMBED_HIDDEN:
        table, (ids,) = rp.embed_case(hidden, 77)
        assert len({int(b) for b in rp.bits(table).flatten()}) == table.numel()
        lst = ids.tolist()
        assert len(lst) == 77 and 0 in lst and rp.EMBED_VOCAB - 1 in lst and min(lst) < 0 and max(lst) >= rp.EMBED_VOCAB
        assert len(set(lst)) < len(lst)
        rows = rp.embed_rows(ids)
        assert rows[lst.index(min(lst))] == 0 and rows[lst.index(max(lst))] == rp.EMBED_VOCAB - 1
        _, singles = rp.embed_case(hidden, 1)
        assert [int(i) for i in singles] == [-3, rp.EMBED_VOCAB, 0, rp.EMBED_VOCAB - 1, 4]


@pytest.mark.parametrize("hidden", rp.POOL_HIDDEN)
def test_pool_probes_equal_the_chain_reference(hidden):
    spans = rp.pool_spans()
    assert [b - a for a, b in spans] == [1, 0, 2, 8, 0] and spans[-1][1] <= rp.N_SIGNS
    assert max(rp.POOL_ROWS) == rp.N_SIGNS - 1 and 0 in rp.POOL_ROWS and len(set(rp.POOL_ROWS)) < len(rp.POOL_ROWS)
    assert hidden in rp.pool_out_dims(hidden) and 1 in rp.pool_out_dims(hidden)
    for with_delta in (False, True):
        p = rp.pool_probe(hidden, with_delta)
        for kw in [dict(dtype=F64)] + [dict(dtype=F32, rstd_scale=s) for s in SCALES]:
            rows = rp.pooled_row_ref(p["hs"], p["w"], [(t, t + 1) for t in range(rp.N_SIGNS)], 0, rp.EPS, p.get("delta"), **kw)
            assert torch.equal(rows, p["normed"])
    toks = rp.pool_mean_tokens(hidden)
    for a, b in spans:
        if b > a:
            acc = torch.zeros(hidden)
            for t in range(a, b):
                acc += toks[t].float()
            assert torch.equal((acc * torch.tensor(1.0 / (b - a), dtype=F32)).double(), toks[a:b].double().mean(0))


@pytest.mark.parametrize("hidden", rp.CHAIN_HIDDEN)
def test_pooled_row_fp32_chains_meet_the_conditions_with_room(hidden):
    hs, delta, w = rp.pool_chain_case(hidden)
    spans = [(t, t + 1) for t in range(rp.N_SIGNS)]
    want = rp.to_bf16(rp.pooled_row_ref(hs, w, spans, 0, rp.EPS, delta))
    for scale in SCALES:
        row = rp.pooled_row_ref(hs, w, spans, 0, rp.EPS, delta, dtype=F32, rstd_scale=scale)
        # what the GPU file does: the fp32 output times the reference's norm, rounded to bf16, gives the row back
        out32 = (row / row.norm(dim=1, keepdim=True)).float()
        back = rp.to_bf16(out32.double() * want.double().norm(dim=1, keepdim=True))
        assert rp.check_chain(back, want, rp.MAX_ULPS, TENTH) <= TENTH
    dropped = rp.to_bf16(rp.pooled_row_ref(hs, w, spans, 0, rp.EPS, delta, dtype=F32, inner=False))
    assert rp.fails_chain(dropped, want)


# ----------------------------------------------------------------------------------------------------------------------
# the heads
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", sorted(set(rp.LM_HIDDEN + rp.RERANK_HIDDEN)))
def test_integer_rows_norm_to_exact_integers(hidden):
    for with_delta in (False, True):
        p = rp.int_rows(8, hidden, with_delta, "host")
        for dtype, scale in [(F64, 1.0)] + [(F32, s) for s in SCALES]:
            out = rp.rmsnorm_chain(p["hs"], p["w"], rp.EPS, p["delta"], dtype=dtype, rstd_scale=scale)[0]
            assert torch.equal(out.double(), p["normed"].double())
    if hidden in rp.LM_HIDDEN:
        lm, want = rp.lm_integer(p, 300)
        assert int(want.abs().max()) < 2 ** 24 and torch.equal(rp.head_ref(p["hs"], p["w"], rp.EPS, lm, p["delta"])[1], want.double())
        cols = rp.lm_one_hot_columns(hidden + 1, hidden)
        assert sorted(set(cols.tolist())) == list(range(hidden))
        hs, w, lm1, want1 = rp.lm_one_hot(hidden, 8, 17)
        assert torch.equal(rp.head_ref(hs, w, rp.EPS, lm1)[1], want1.double())
    if hidden in rp.RERANK_HIDDEN:
        for kind, d in (("equal", 0), ("plus200", 200), ("minus200", -200)):
            lmr = rp.rerank_lm(p, kind)
            dots = p["normed"][-1].double() @ lmr.double().t()
            assert float(dots[0] - dots[1]) == d, kind
        assert float(rp.score_ref(torch.tensor(0.0), torch.tensor(0.0))) == 0.5
        assert float(rp.score_ref(torch.tensor(100.0), torch.tensor(-100.0)).float()) == 1.0
        assert 0 < float(rp.score_ref(torch.tensor(-100.0), torch.tensor(100.0))) < 1e-80


def test_argmax_cases_hold_what_their_names_promise():
    seen = set()
    for c in rp.argmax_cases():
        logits = rp.head_ref(c["hs"], c["w"], rp.EPS, c["lm"])[1]
        tokens = rp.argmax_ref(logits, c["banned"])
        finite = torch.isfinite(logits)
        assert bool((logits[finite] == logits[finite].round()).all()) and float(logits[finite].abs().max()) < 2 ** 24
        name, vocab = c["name"], logits.shape[1]
        seen.add(name.split(",")[0])
        if name == "all-NaN row":
            assert bool(torch.isnan(logits[3]).all()) and tokens[3] == -1 and all(t >= 0 for i, t in enumerate(tokens) if i != 3)
        elif name == "every finite id banned":
            assert tokens == [-1] * 8 and bool(torch.isnan(logits[:, [2, 5]]).all()) and int(finite.sum()) == 8 * 13
        elif name == "-inf but one":
            assert tokens == [11] * 8 and int(finite.sum()) == 8 and bool((logits[~finite] == -math.inf).all())
        elif name.startswith("maximum at the ends"):
            assert tokens == [0 if r % 2 == 0 else vocab - 1 for r in range(8)]
        else:
            for r, (a, b) in enumerate(c["pairs"]):
                live = [i for i in (a, b) if i not in c["banned"]]
                assert logits[r, a] == logits[r, b] == 72 and tokens[r] == min(live)
            assert vocab in (1023, 1024, 1025)
    assert seen == {"all-NaN row", "every finite id banned", "-inf but one", "maximum at the ends", "ties"}
