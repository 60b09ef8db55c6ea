"""What the GEMM probes (tests/gemm_probes.py) rest on, for every case tests/test_gemm_probes_gpu.py runs, on the CPU: the
exact sums are bf16 values (so equality with the int64 matmul is the comparison, not a tolerance), the weight orders of
encoder/ops.py are the header's index formulas, every class of fault moves the reference of every integer case, the
selection columns hold the edges of each form's K division, and the prologue's documented arithmetic gives +-norm_w."""
from __future__ import annotations

import pytest
import torch

import gemm_probes as gp

NAN = float("nan")
FORMS = gp.SKINNY_FORMS + gp.SMALL_FORMS


def _exact(op, swiglu):
    ref = op.ref2.double() / 2
    assert float(ref.abs().max()) <= gp.REF_LIMIT
    assert torch.equal(ref.float().to(gp.BF).float().double(), ref)
    assert torch.equal(op.ref2, gp.int_reference(op.xop2, op.w))
    if swiglu:
        assert float(ref[:, : ref.shape[1] // 2].abs().max()) <= gp.GATE_LIMIT
    return float(ref.abs().max())


def _sparse_rows_hit(op, mode, ranges):
    """Exactly 24 non-zeros in every row of the sparse operand, some in every K range."""
    sparse = op.xop2 if mode == "dense_w" else op.w
    nz = sparse != 0
    assert bool((nz.sum(1) == gp.NNZ).all())
    for lo, hi in ranges:
        assert bool(nz[:, lo:hi].any(1).all()), (lo, hi)


def _wide_cases():
    for k, splitk in gp.WIDE_K_SPLITS:
        for n in gp.WIDE_NS:
            yield k, splitk, n, [m for m, _ in gp.WIDE_ROWS]
    yield gp.WIDE_4B[0], gp.WIDE_4B[1], gp.WIDE_4B[2], [m for m, _ in gp.WIDE_ROWS]
    for k, splitk, n in gp.WIDE_THRESHOLD:
        yield k, splitk, n, [64]


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f.name)
def test_form_integer_cases_are_exact_and_bite(form):
    worst, count = 0.0, 0
    for n in gp.form_ns(form, gp.NOMINAL_CUS):
        for mode in gp.form_modes(form):
            op = gp.form_operands(form, n, mode)
            worst = max(worst, _exact(op, form.swiglu))
            for m_pad, rows in gp.SMALL_ROWS:
                ranges = gp.form_ranges(form, m_pad)
                assert ranges[0][0] == 0 and ranges[-1][1] == form.k
                _sparse_rows_hit(op, mode, ranges)
                for m_rows in rows:
                    got = gp.bites(op, m_rows, m_pad, ranges, 32, 32, gp.tile_features(form.family, form.rows, form.swiglu),
                                   form.swiglu, NAN)
                    want = {"zero_step", "move_split", "swap_rows"} | ({"swap_gate_up"} if form.swiglu else set()) \
                        | ({"pad_row"} if m_rows < m_pad else set())
                    assert set(got) == want and all(got.values()), (n, mode, m_pad, m_rows, got)
                    count += 1
    print(f"\n{form.name}: {count} cases, every fault bites, max |ref| = {worst}")


@pytest.mark.parametrize("tile,chunk", gp.WIDE_TILES)
def test_wide_integer_cases_are_exact_and_bite(tile, chunk):
    worst, count = 0.0, 0
    for k, splitk, n, m_pads in _wide_cases():
        ranges = gp.split_ranges(k, splitk, chunk)
        assert ranges[0][0] == 0 and ranges[-1][1] == k and 1 <= splitk <= k // 128
        for mode in gp.MODES:
            op = gp.wide_operands(k, n, mode)
            worst = max(worst, _exact(op, True))
            if k // 64 <= 20:
                _sparse_rows_hit(op, mode, [(c, c + 64) for c in range(0, k, 64)])
            for swiglu in (False, True):
                for m_pad in m_pads:
                    for m_rows in dict(gp.WIDE_ROWS)[m_pad]:
                        got = gp.bites(op, m_rows, m_pad, ranges, 16, chunk, gp.tile_features("wide", 32, swiglu), swiglu,
                                       gp.WIDE_PAD_VALUE)
                        want = {"zero_step", "move_split", "swap_rows"} | ({"swap_gate_up"} if swiglu else set()) \
                            | ({"pad_row"} if m_rows < m_pad else set())
                        assert set(got) == want and all(got.values()), (k, splitk, n, mode, swiglu, m_pad, m_rows, got)
                        count += 1
    print(f"\ntile {tile}: {count} cases, every fault bites, max |ref| = {worst}")


def test_wide_case_table_reaches_one_two_three_even_and_odd_chunks_per_split():
    seen = {}
    for tile, chunk in gp.WIDE_TILES:
        per = set()
        for k, splitk in gp.WIDE_K_SPLITS + (gp.WIDE_4B[:2],):
            per.update(gp.wide_chunks_per_split(k, splitk, chunk))
        seen[tile] = per
    assert {1, 2, 3, 9, 10} <= seen[128] and {2, 3, 4, 5, 6, 19} <= seen[64]      # (a 64-column chunk: never 1 per split)
    assert [gp.wide_default_tile(n, s) for _, s, n in gp.WIDE_THRESHOLD] == [128, 64]


def test_many_tile_case_does_not_divide_over_the_workgroups():
    for form in gp.SMALL_FORMS:
        ns = gp.small_ns(form, gp.NOMINAL_CUS)
        assert ns[:2] == (form.rows, 3 * form.rows) and (len(ns) == 3) == form.multi
        if form.multi:
            tiles = ns[2] // form.rows
            assert tiles > gp.NOMINAL_CUS and tiles % gp.NOMINAL_CUS


def test_weight_orders_match_the_header_formulas():
    """encoder/ops.py's view/permute against the index formulas, on weights whose value is their own (row, column)."""
    from cadence_rag_amd.encoder import ops
    shapes = {(n, f.k) for f in FORMS for n in gp.form_ns(f, gp.NOMINAL_CUS)}
    for n, k in sorted(shapes):
        w = torch.arange(n * k, dtype=torch.int32).view(n, k)
        if n % 16 == 0:
            assert torch.equal(ops.skinny_weight(w).flatten(), gp.skinny_weight(w))
            assert torch.equal(ops.skinny_gate_up_weight(w).flatten(), gp.skinny_gate_up_weight(w))
        for rows in (10, 12, 16):
            if n % rows == 0:
                assert torch.equal(ops.small_weight(w, rows).flatten(), gp.small_weight(w, rows))
    for k, n in sorted({(k, n) for k, _, n, _ in _wide_cases()}):
        w = torch.arange(n * k, dtype=torch.int32).view(n, k)
        assert torch.equal(ops.wide_weight(w).flatten(), gp.wide_weight(w))
        assert torch.equal(ops.wide_gate_up_weight(w).flatten(), gp.wide_gate_up_weight(w))
    # and as the kernels are fed: two bf16-exact integers per element, carried in two tensors
    n, k = 256, 256
    row = torch.arange(n, dtype=torch.float32)[:, None].expand(n, k).to(gp.BF).contiguous()
    col = torch.arange(k, dtype=torch.float32)[None, :].expand(n, k).to(gp.BF).contiguous()
    for mine, theirs in ((gp.skinny_weight, ops.skinny_weight), (gp.skinny_gate_up_weight, ops.skinny_gate_up_weight),
                         (gp.wide_weight, ops.wide_weight), (gp.wide_gate_up_weight, ops.wide_gate_up_weight)):
        assert torch.equal(theirs(row).flatten(), mine(row)) and torch.equal(theirs(col).flatten(), mine(col))


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f.name)
def test_form_selection_columns_hold_every_wave_edge(form):
    cols = gp.form_select_columns(form)
    assert cols == sorted(set(cols)) and 0 <= cols[0] and cols[-1] == form.k - 1
    for m_pad, divs in form.division:
        for waves, ks in divs:
            assert waves * ks * 32 == form.k
            for w in range(waves):
                assert 32 * ks * w in cols and 32 * ks * (w + 1) - 1 in cols
    mid = [c for c in range(0, form.k, 32) if all(c + j in cols for j in range(32))]
    assert mid and 0 < mid[0] < form.k - 32                      # all 32 positions 8 g + e of a middle k-step
    for m_pad, rows in gp.SMALL_ROWS:
        for m_rows in rows:
            launches = gp.selection_launches(cols, m_rows)
            assert all(len(g) == m_rows for g in launches) and {c for g in launches for c in g} == set(cols)
            x = gp.one_hot(launches[0], m_pad, form.k, NAN)
            assert bool((x[:m_rows].float().sum(1) == 1).all()) and bool(torch.isnan(x[m_rows:].float()).all())


@pytest.mark.parametrize("k,splitk", gp.WIDE_K_SPLITS)
def test_wide_selection_columns_hold_every_split_and_chunk_edge(k, splitk):
    cols = gp.wide_select_columns(k, splitk)
    for tile, chunk in gp.WIDE_TILES:
        chunks = k // chunk
        for c in range(chunks):
            assert chunk * c in cols and chunk * (c + 1) - 1 in cols
        for s in range(splitk):
            assert chunk * (chunks * s // splitk) in cols and chunk * (chunks * (s + 1) // splitk) - 1 in cols
    mid = [c for c in range(0, k, 16) if all(c + j in cols for j in range(16))]     # both halves h of a 16-wide step
    assert mid


def test_swiglu_set_brackets_silu():
    g = torch.cat([torch.arange(-160, 161) / 2, torch.randn(4096) * 0.02]).to(gp.BF)
    lo, hi = gp.silu_neighbours(g)
    s = g.double() / (1 + torch.exp(-g.double()))
    assert bool((lo.double() <= s).all()) and bool((s <= hi.double()).all())
    step = gp._bf16_step(lo, up=True)
    assert bool(((hi == lo) | (hi == step)).all())               # equal, or adjacent bf16 values
    assert bool(((lo == hi) == (lo.double() == s)).all())


@pytest.mark.parametrize("form", [f for f in gp.SMALL_FORMS if f.prologue], ids=lambda f: f.name)
def test_prologue_probes_give_plus_minus_norm_w(form):
    for n in gp.form_ns(form, gp.NOMINAL_CUS):
        op = gp.form_operands(form, n, "prologue")
        s = op.x.double() + op.delta.double()
        c = s.abs()
        assert bool((c == c[:, :1]).all()) and bool((torch.log2(c[:, 0]) % 1 == 0).all())   # |x + delta| = c, a power of two
        assert torch.equal(op.res.double(), s)
        want = op.xop2.double() / 2
        assert bool((want.abs() == op.norm_w.double().abs()).all())
        for err in (0.0, 2.0 ** -12, -(2.0 ** -12)):             # rsqrtf is good to ~2^-22; half a bf16 ulp is 2^-9
            assert torch.equal(gp.prologue_operand(op.x, op.delta, op.norm_w, err).double(), want)
