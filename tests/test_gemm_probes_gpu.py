"""Exact probes through the encoder's GEMM kernels (construction, references, case lists: tests/gemm_probes.py; the
conditions that make equality the right comparison are proven for every case by tests/test_gemm_probes_host.py).

Every comparison is equality: an integer probe's output must equal the int64 matmul, a selection probe's output row must
be the weight column bit for bit, a SwiGLU output must be a member of the one- or two-element set the exact gate and up
sums admit AND carry the bits of crag_enc_swiglu on the exact gate|up matrix.  Sentinels (7.0 behind bf16 outputs, NaN
behind fp32 scratch) are checked after every call.

Kernels reached: skinny_gemm_kernel<1|2, 2, 10, 8, 0|1>, <1|2, 1, 16, 8, 0>, <1, 1, 38, 8, 0>, <2, 1, 19, 16, 0>;
small_gemm_kernel<1|2, 10, 8, 10, 12, 0, 1, 1, 1>, <1|2, 10, 8, 10, 16, 1, 1, 1, 1>, <1|2, 16, 8, 16, 10, 0, 0, 0, 1>,
<1, 38, 8, 19, 10, 0, 0, 0, 1>, <2, 38, 8, 12, 10, 0, 0, 0, 2>; wide_gemm_kernel<1|2|3|4, 4, 8> and <1|2|3|4, 2, 4> with
partial tiles, token-major rows and direct output; wide_reduce_kernel (both epilogues); rmsnorm_partials_kernel."""
from __future__ import annotations

import pytest
import torch

import gemm_probes as gp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF = torch.bfloat16
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int16)


class Tally:
    """Comparisons stay on the device until check(): one synchronisation per group of launches."""

    def __init__(self):
        self.items = []

    def add(self, label, ok):
        self.items.append((label, ok.all() if ok.dim() else ok))

    def same(self, label, got, want):
        self.add(label, _bits(got) == _bits(want))

    def check(self):
        if not self.items:
            return
        flags = torch.stack([ok for _, ok in self.items]).cpu().tolist()
        bad = [label for (label, _), ok in zip(self.items, flags) if not ok]
        self.items = []
        assert not bad, f"{len(bad)} comparisons failed; first: {bad[:8]}"


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _swiglu_bits(pre):
    """crag_enc_swiglu on the exact bf16 gate|up matrix [m, 2 I]."""
    from cadence_rag_amd.encoder import ops
    out = torch.empty(pre.shape[0], pre.shape[1] // 2, dtype=BF, device=DEV)
    return ops.swiglu(pre.contiguous(), out)


class Expect:
    """The exact pre-activation rows [rows, n] (bf16) and, for SwiGLU, the admissible set of every row, on the device."""

    def __init__(self, pre_cpu):
        self.pre = pre_cpu.to(DEV)
        inter = pre_cpu.shape[1] // 2
        self.lo, self.hi = (t.to(DEV) for t in gp.swiglu_set(pre_cpu[:, :inter], pre_cpu[:, inter:]))


def _check_output(tally, label, out, m_rows, exp, sel, swiglu):
    """out [m_pad + 1, width] against rows `sel` (a slice or an index tensor) of the expectation: rows behind m_rows keep
    their sentinel; plain outputs are the exact sums to the bit; SwiGLU outputs lie in the admissible set and carry
    crag_enc_swiglu's bits."""
    tally.add(label + " sentinel", out[m_rows:] == 7.0)
    got = out[:m_rows]
    if not swiglu:
        tally.same(label, got, exp.pre[sel])
        return
    tally.add(label + " set", gp.member(got, exp.lo[sel], exp.hi[sel]))
    tally.same(label + " swiglu bits", got, _swiglu_bits(exp.pre[sel]))


# ----------------------------------------------------------------------------------------------------------------------
# skinny and small
# ----------------------------------------------------------------------------------------------------------------------
def _form_weight(form, w):
    from cadence_rag_amd.encoder import ops
    if form.swiglu:
        return ops.skinny_gate_up_weight(w)          # (small_weight(., 16) is skinny_weight's order)
    return ops.skinny_weight(w) if form.family == "skinny" else ops.small_weight(w, form.rows)


def _form_launch(form, x, wsw, out, m_rows, n, pro=None):
    from cadence_rag_amd.encoder import ops
    if form.family == "skinny":
        return ops.skinny_gemm(x, wsw, out, m_rows, n, swiglu=form.swiglu)
    kw = {} if pro is None else dict(delta=pro[0], norm_w=pro[1], res_out=pro[2], eps=gp.EPS)
    return ops.small_gemm(x, wsw, out, m_rows, n, form.rows, swiglu=form.swiglu, **kw)


def _run_form_integer(form, m_pad):
    tally = Tally()
    for n in gp.form_ns(form, _cus()):
        for mode in gp.form_modes(form):
            op = gp.form_operands(form, n, mode)
            wsw = _form_weight(form, op.w.to(DEV))
            exp = Expect(gp.pre_activation(op.ref2))
            width = n // 2 if form.swiglu else n
            for m_rows in dict(gp.SMALL_ROWS)[m_pad]:
                label = f"{form.name} n={n} {mode} m_rows={m_rows}/{m_pad}"
                x = gp.padded(op.x, m_rows, m_pad, NAN).to(DEV)
                out = torch.full((m_pad + 1, width), 7.0, dtype=BF, device=DEV)
                if form.prologue:
                    delta = gp.padded(op.delta, m_rows, m_pad, NAN).to(DEV)
                    x0, d0 = x.clone(), delta.clone()
                    res = torch.full((m_pad, form.k), 7.0, dtype=BF, device=DEV)
                    _form_launch(form, x, wsw, out, m_rows, n, pro=(delta, op.norm_w.to(DEV), res))
                    tally.same(label + " res_out", res[:m_rows], op.res[:m_rows].to(DEV))
                    tally.add(label + " res_out rows behind m_rows", res[m_rows:] == 7.0)
                    tally.same(label + " x unmodified", x, x0)
                    tally.same(label + " delta unmodified", delta, d0)
                else:
                    _form_launch(form, x, wsw, out, m_rows, n)
                _check_output(tally, label, out, m_rows, exp, slice(0, m_rows), form.swiglu)
            tally.check()


def _run_form_selection(form, m_pad):
    tally = Tally()
    cols = gp.form_select_columns(form)
    for n in gp.form_ns(form, _cus()):
        w = gp.selection_weight(n, form.k, seed=n + form.k).to(DEV)
        wsw = _form_weight(form, w)
        exp = Expect(w.t().contiguous().cpu())
        width = n // 2 if form.swiglu else n
        for m_rows in dict(gp.SMALL_ROWS)[m_pad]:
            rows = torch.arange(m_rows, device=DEV)
            for i, grp in enumerate(gp.selection_launches(cols, m_rows)):
                idx = torch.tensor(grp, device=DEV)
                x = torch.zeros(m_pad, form.k, dtype=BF, device=DEV)
                x[m_rows:] = NAN
                x[rows, idx] = 1.0
                out = torch.full((m_pad + 1, width), 7.0, dtype=BF, device=DEV)
                _form_launch(form, x, wsw, out, m_rows, n)
                _check_output(tally, f"{form.name} n={n} m_rows={m_rows}/{m_pad} columns {grp[:4]}..", out, m_rows, exp, idx,
                              form.swiglu)
            tally.check()


@pytest.mark.parametrize("m_pad", [16, 32])
@pytest.mark.parametrize("form", gp.SKINNY_FORMS, ids=lambda f: f.name)
def test_skinny_gemm_integer_probes(gpu, form, m_pad):
    _run_form_integer(form, m_pad)


@pytest.mark.parametrize("m_pad", [16, 32])
@pytest.mark.parametrize("form", gp.SKINNY_FORMS, ids=lambda f: f.name)
def test_skinny_gemm_selection_probes(gpu, form, m_pad):
    _run_form_selection(form, m_pad)


@pytest.mark.parametrize("m_pad", [16, 32])
@pytest.mark.parametrize("form", gp.SMALL_FORMS, ids=lambda f: f.name)
def test_small_gemm_integer_and_prologue_probes(gpu, form, m_pad):
    """The prologue forms run the equal-magnitude probes (res_out exact, its rows behind m_rows untouched, x and delta
    unmodified); the many-tile n gives the grid-stride walk a tile count the workgroups do not divide."""
    _run_form_integer(form, m_pad)


@pytest.mark.parametrize("m_pad", [16, 32])
@pytest.mark.parametrize("form", [f for f in gp.SMALL_FORMS if not f.prologue], ids=lambda f: f.name)
def test_small_gemm_selection_probes(gpu, form, m_pad):
    _run_form_selection(form, m_pad)


# ----------------------------------------------------------------------------------------------------------------------
# the wide family
# ----------------------------------------------------------------------------------------------------------------------
class Wide:
    """One (x, W) pair through an entry point of the wide family; sentinels behind every buffer."""

    def __init__(self, lib, tally):
        from cadence_rag_amd import _native
        from cadence_rag_amd.encoder import ops
        self.lib, self.tally, self.ops, self.check = lib, tally, ops, _native.check
        self.scratch = torch.empty(0, dtype=torch.float32, device=DEV)

    def weights(self, w):
        """(plain order, gate|up order) of a torch-layout weight on the device."""
        return self.ops.wide_weight(w), self.ops.wide_gate_up_weight(w)

    def _scratch(self, m_pad, n, splitk):
        need = self.lib.crag_enc_wide_partial_bytes(m_pad, n, splitk) // 4
        assert need == splitk * n * m_pad
        if self.scratch.numel() < need + 64:
            self.scratch = torch.empty(need + 64, dtype=torch.float32, device=DEV)
        s = self.scratch[:need + 64]
        s.fill_(NAN)
        return s, need

    def run(self, label, entry, x, ww, m_rows, n, splitk, exp, sel, resid=None, norm_w=None):
        """exp[sel]: the exact pre-activation of the m_rows rows (for "rows": the exact delta)."""
        p, st, lib, tally = self.ops._p, self.ops._stream(), self.lib, self.tally
        m_pad, k = x.shape
        label = f"{label} {entry}"
        if entry == "rows":
            pre = exp.pre[sel].contiguous()
            s, need = self._scratch(m_pad, n, splitk)
            self.check(lib.crag_enc_wide_gemm_rows(p(x), p(ww), p(s), m_pad, n, k, splitk, st), "crag_enc_wide_gemm_rows")
            tally.add(label + " scratch tail", torch.isnan(s[need:]))
            parts = s[:need].view(splitk, m_pad, n)
            if resid is None:                      # selection: one split holds the weight column, the others +-0
                tally.add(label + " partial rows", parts[:, :m_rows].sum(0) == pre.float())
                return
            want_norm, want_res = torch.empty_like(pre), torch.empty_like(pre)
            self.ops.rmsnorm(pre, norm_w, want_norm, gp.EPS, residual_in=resid[:m_rows].contiguous(), residual_out=want_res)
            tally.same(label + " exact residual", want_res, (resid[:m_rows].float() + pre.float()).to(BF))
            res_io = resid.clone()                 # residual_out aliases residual_in, as in the forward
            normed = torch.full((m_rows + 1, n), 7.0, dtype=BF, device=DEV)
            self.ops.rmsnorm_partials(s, splitk, m_pad, norm_w, normed[:m_rows], gp.EPS, residual_in=res_io, residual_out=res_io)
            tally.same(label + " residual", res_io[:m_rows], want_res)
            tally.same(label + " residual rows behind m_rows", res_io[m_rows:], resid[m_rows:])
            tally.same(label + " normed", normed[:m_rows], want_norm)
            tally.add(label + " normed sentinel", normed[m_rows] == 7.0)
            return
        kind, epilogue = entry.split("-")
        epilogue = int(epilogue)
        out = torch.full((m_pad + 1, n // 2 if epilogue else n), 7.0, dtype=BF, device=DEV)
        if kind == "direct":
            self.check(lib.crag_enc_wide_gemm_direct(p(x), p(ww), p(out), m_rows, m_pad, n, k, epilogue, st),
                       "crag_enc_wide_gemm_direct")
        else:
            s, need = self._scratch(m_pad, n, splitk)
            self.check(lib.crag_enc_wide_gemm(p(x), p(ww), p(s), m_pad, n, k, splitk, st), "crag_enc_wide_gemm")
            self.check(lib.crag_enc_wide_reduce(p(s), p(out), m_rows, m_pad, n, splitk, epilogue, st), "crag_enc_wide_reduce")
            tally.add(label + " scratch tail", torch.isnan(s[need:]))
        _check_output(tally, label, out, m_rows, exp, sel, bool(epilogue))


def _wide_integer(wide, k, splitk, n, m_pads, tile):
    """Both integer modes through every entry point the split allows, at every (m_pad, m_rows)."""
    tally = wide.tally
    g = torch.Generator().manual_seed(k + n)
    resid_all = torch.randint(-8, 9, (128, n), generator=g).to(BF).to(DEV)
    norm_w = (1 + 0.1 * torch.randn(n, generator=g)).to(BF).to(DEV)
    for mode in gp.MODES:
        op = gp.wide_operands(k, n, mode)
        weights = wide.weights(op.w.to(DEV))
        exp = Expect(gp.pre_activation(op.ref2))
        for m_pad in m_pads:
            for m_rows in dict(gp.WIDE_ROWS)[m_pad]:
                label = f"tile={tile} k={k} splitk={splitk} n={n} {mode} m_rows={m_rows}/{m_pad}"
                for entry in gp.wide_entries(splitk):
                    if entry == "rows" and n > 4096:       # (crag_enc_rmsnorm_partials: hidden <= 4096)
                        continue
                    x = gp.padded(op.x, m_rows, m_pad, gp.WIDE_PAD_VALUE).to(DEV)
                    wide.run(label, entry, x, weights[1 if entry.endswith("-1") else 0], m_rows, n, splitk, exp,
                             slice(0, m_rows), resid=resid_all[:m_pad].contiguous(), norm_w=norm_w)
            tally.check()


def _wide_selection(wide, k, splitk, n, m_pad, tile):
    tally = wide.tally
    cols = gp.wide_select_columns(k, splitk)
    w = gp.selection_weight(n, k, seed=n + k).to(DEV)
    plain, gate_up = wide.weights(w)
    exp = Expect(w.t().contiguous().cpu())
    for m_rows in dict(gp.WIDE_ROWS)[m_pad]:
        rows = torch.arange(m_rows, device=DEV)
        for grp in gp.selection_launches(cols, m_rows):
            idx = torch.tensor(grp, device=DEV)
            x = torch.zeros(m_pad, k, dtype=BF, device=DEV)
            x[m_rows:] = gp.WIDE_PAD_VALUE
            x[rows, idx] = 1.0
            label = f"tile={tile} k={k} splitk={splitk} n={n} m_rows={m_rows}/{m_pad} columns {grp[:4]}.."
            for entry in gp.wide_entries(splitk):
                wide.run(label, entry, x, gate_up if entry.endswith("-1") else plain, m_rows, n, splitk, exp, idx)
        tally.check()


@pytest.mark.parametrize("m_pad", [32, 64, 96, 128])
@pytest.mark.parametrize("tile", [t for t, _ in gp.WIDE_TILES])
def test_wide_gemm_integer_probes(gpu, monkeypatch, tile, m_pad):
    """1, 2, 3, even and odd chunks per split (prologue only, odd tail, clamped re-loads) under both tile shapes, through
    partial tiles + reduce, the direct form and token-major rows + rmsnorm_partials."""
    monkeypatch.setenv("CRAG_WIDE_TILE", str(tile))
    wide = Wide(gpu, Tally())
    for k, splitk in gp.WIDE_K_SPLITS:
        for n in gp.WIDE_NS:
            _wide_integer(wide, k, splitk, n, (m_pad,), tile)


@pytest.mark.parametrize("m_pad", [32, 64, 96, 128])
@pytest.mark.parametrize("tile", [t for t, _ in gp.WIDE_TILES])
def test_wide_gemm_selection_probes(gpu, monkeypatch, tile, m_pad):
    monkeypatch.setenv("CRAG_WIDE_TILE", str(tile))
    wide = Wide(gpu, Tally())
    for k, splitk in gp.WIDE_K_SPLITS:
        for n in gp.WIDE_NS:
            _wide_selection(wide, k, splitk, n, m_pad, tile)


@pytest.mark.parametrize("tile", [t for t, _ in gp.WIDE_TILES])
def test_wide_gemm_integer_probes_at_the_4b_down_projection(gpu, monkeypatch, tile):
    """(k 9728, splitk 8, n 2560): 76 chunks of 128 split as 9 or 10."""
    monkeypatch.setenv("CRAG_WIDE_TILE", str(tile))
    k, splitk, n = gp.WIDE_4B
    _wide_integer(Wide(gpu, Tally()), k, splitk, n, [m for m, _ in gp.WIDE_ROWS], tile)


@pytest.mark.parametrize("k,splitk,n", gp.WIDE_THRESHOLD)
def test_wide_gemm_is_exact_on_both_sides_of_the_tile_threshold(gpu, monkeypatch, k, splitk, n):
    """Without the developer switch: (n / 128) * splitk = 100 takes 128-row tiles, 99 takes 64-row tiles."""
    monkeypatch.delenv("CRAG_WIDE_TILE", raising=False)
    assert gp.wide_default_tile(n, splitk) == (128 if (n // 128) * splitk == 100 else 64)
    _wide_integer(Wide(gpu, Tally()), k, splitk, n, (64,), "default")
