"""crag_enc_logprobs on the GPU, through ops.logprobs, against the host rule (cadence_rag_amd.logprobs.logprobs_host).

Exact, no tolerance: rank, top_id and the padding, on rows with the token at id 0 and at vocab - 1, duplicated maxima,
+-0, NaN and -inf entries, n_top == vocab and fewer candidates than n_top; infinite and NaN floats; the same bits for a
row alone, as row 0 of 8 and as row 7 of 8.
Floats (logprob, lse_all, lse_allowed, top_logprob): |kernel - fp64 rule| <= logprobs.error_bar = 2^-24 (24 + 4 |ln Z| +
|lse| + |value|), the bound DESIGN 6d derives from the fp32 subtractions, expf / logf, the fixed-point truncation and the
final roundings -- fixed before the kernel ran, not read off it.
The sizes are test_sample_gpu.py's word, wave and workgroup edges; 4096 / 4097 equal logits sit on the two sides of the
kernel's LDS capacity, where it changes from counting inside LDS to rounds over the row."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest
import torch

from cadence_rag_amd.logprobs import MAX_TOP, error_bar, logprobs_host

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SIZES = [1, 31, 33, 63, 64, 65, 1023, 1024, 1025, 4097, 151_936]
FLOAT_FILL, INT_FILL = 123.0, -7
NAN = float("nan")


def _pack(allowed: np.ndarray) -> torch.Tensor:
    """bool [n, V] -> int32 [n, ceil(V / 32)], bit t % 32 of word t / 32."""
    n, v = allowed.shape
    padded = np.zeros((n, (v + 31) // 32 * 32), np.uint8)
    padded[:, :v] = allowed
    words = np.packbits(padded, axis=1, bitorder="little").view(np.uint32)
    return torch.from_numpy(words.view(np.int32).copy()).to(DEV)


def _run(logits: np.ndarray, tokens, allowed=None, n_top=0):
    """One call: the outputs as host tensors, every one filled with a sentinel first."""
    from cadence_rag_amd.encoder import ops
    n = logits.shape[0]
    lg = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).to(DEV)
    tok = torch.tensor([int(t) for t in tokens], dtype=torch.int32).to(DEV)
    f = lambda *shape: torch.full(shape, FLOAT_FILL, dtype=torch.float32, device=DEV)   # noqa: E731
    i = lambda *shape: torch.full(shape, INT_FILL, dtype=torch.int32, device=DEV)       # noqa: E731
    out = {"logprob": f(n), "lse_all": f(n), "lse_allowed": f(n), "rank": i(n),
           "top_id": i(n, n_top) if n_top else None, "top_logprob": f(n, n_top) if n_top else None}
    ops.logprobs(lg, tok, out["logprob"], allowed_bits=None if allowed is None else _pack(allowed),
                 lse_all=out["lse_all"], lse_allowed=out["lse_allowed"], rank=out["rank"], top_id=out["top_id"],
                 top_logprob=out["top_logprob"])
    torch.cuda.synchronize()
    return {k: (None if t is None else t.cpu()) for k, t in out.items()}


def _close(got: float, want: float, lse: float, ln_z: float, what: str, worst: dict) -> None:
    if math.isnan(want) or math.isinf(want):
        assert (math.isnan(got) and math.isnan(want)) or got == want, f"{what}: {got} for {want}"
        return
    bar = error_bar(want, lse, ln_z)
    err = abs(float(got) - want)
    worst["ratio"] = max(worst.get("ratio", 0.0), err / bar)
    assert err <= bar, f"{what}: {got} for {want}: |d| = {err:.3e} > bar {bar:.3e}"


def _check_row(out, r, row, token, allowed, n_top, worst) -> None:
    want = logprobs_host(row, token, allowed, n_top)
    assert int(out["rank"][r]) == want.rank, f"rank of row {r}"
    _close(float(out["lse_all"][r]), want.lse_all, want.lse_all, want.ln_z_all, f"lse_all[{r}]", worst)
    _close(float(out["lse_allowed"][r]), want.lse_allowed, want.lse_allowed, want.ln_z_allowed, f"lse_allowed[{r}]", worst)
    _close(float(out["logprob"][r]), want.logprob, want.lse_all, want.ln_z_all, f"logprob[{r}]", worst)
    if n_top:
        assert out["top_id"][r].tolist() == want.top_id.tolist(), f"top ids of row {r}"
        for k in range(n_top):
            _close(float(out["top_logprob"][r, k]), float(want.top_logprob[k]), want.lse_all, want.ln_z_all,
                   f"top_logprob[{r}, {k}]", worst)


def _coarse(rng, v, sd=3.0):
    """Logits on a grid of 1/4: equal values everywhere, at the maximum too."""
    return (np.round(rng.standard_normal(v) * sd * 4) / 4).astype(np.float32)


def _cases(rng, v):
    """Eight (row, token, allowed) of length v: the kinds the module docstring lists."""
    rows = []
    a = (rng.standard_normal(v) * 2).astype(np.float32)                 # N(0, 4)
    rows.append((a, int(rng.integers(0, v)), rng.random(v) < 0.5))
    b = (rng.standard_normal(v) * 30).astype(np.float32)                # weights far below the fixed-point unit
    rows.append((b, int(np.argmax(b)), rng.random(v) < 0.9))
    c = _coarse(rng, v)                                                 # duplicated maxima, the token at id 0
    c[rng.integers(0, v, max(v // 8, 1))] = c.max()
    rows.append((c, 0, rng.random(v) < 0.5))
    d = _coarse(rng, v, 0.5)                                            # +-0 everywhere, the token a zero at vocab - 1
    d[d == 0] = np.where(rng.random(int((d == 0).sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    d[v - 1] = np.float32(-0.0)
    rows.append((d, v - 1, rng.random(v) < 0.5))
    e = (rng.standard_normal(v) * 2).astype(np.float32)                 # NaN and -inf entries, the token a -inf one
    e[rng.random(v) < 0.2] = np.nan
    e[rng.random(v) < 0.2] = -np.inf
    t = int(rng.integers(0, v))
    e[t] = -np.inf
    rows.append((e, t, rng.random(v) < 0.7))
    f = np.full(v, np.nan, np.float32)                                  # fewer candidates than n_top
    some = rng.choice(v, min(v, 5), replace=False)
    f[some] = (rng.standard_normal(some.size) * 2).astype(np.float32)
    rows.append((f, int(some[0]), rng.random(v) < 0.5))
    g = (rng.standard_normal(v) * 2).astype(np.float32)                 # the allowed ids all >= 40 below the maximum
    low = rng.random(v) < 0.3
    low[int(rng.integers(0, v))] = True
    g[low] -= 60.0
    rows.append((g, int(np.nonzero(low)[0][0]), low))
    h = (rng.standard_normal(v) * 30).astype(np.float32)                # a wide row under a thin mask
    rows.append((h, int(rng.integers(0, v)), rng.random(v) < 0.05))
    return rows


@pytest.mark.parametrize("rows", [1, 8])
@pytest.mark.parametrize("v", SIZES)
def test_rows_against_the_host_rule(gpu, v, rows):
    rng = np.random.default_rng(v * 10 + rows)
    cases = _cases(rng, v)
    worst: dict = {}
    tops = sorted({0, min(MAX_TOP, v), min(3, v)})      # n_top == vocab for vocab <= 16
    calls = [cases] if rows == 8 else [[c] for c in cases]
    for call in calls:
        logits = np.stack([c[0] for c in call])
        tokens = [c[1] for c in call]
        masks = np.stack([c[2] for c in call])
        for n_top in tops:
            for allowed in (None, masks):
                out = _run(logits, tokens, allowed, n_top)
                for r, (row, token, mask) in enumerate(call):
                    _check_row(out, r, row, token, None if allowed is None else mask, n_top, worst)
    print(f"vocab {v}, rows {rows}: largest |d| / bar = {worst.get('ratio', 0.0):.3f}")


def test_the_two_maxima(gpu):
    """The allowed ids all lie >= 40 below the global maximum: relative to m_all every allowed weight is below e^-40,
    far under the fixed-point unit 2^-40; lse_allowed is taken relative to m_alw and stays finite and inside the bar."""
    rng = np.random.default_rng(3)
    v = 4097
    row = (rng.standard_normal(v) * 2).astype(np.float32)
    mask = np.zeros(v, bool)
    mask[rng.choice(v, 300, replace=False)] = True
    row[mask] -= 40.0 + float(row.max() - row.min())
    assert float(row[~mask].max() - row[mask].max()) >= 40.0
    out = _run(row[None], [int(np.nonzero(mask)[0][0])], mask[None], 4)
    assert math.isfinite(float(out["lse_allowed"][0]))
    _check_row(out, 0, row, int(np.nonzero(mask)[0][0]), mask, 4, {})
    assert float(out["lse_allowed"][0]) - float(out["lse_all"][0]) < -39.0


@pytest.mark.parametrize("v", [4096, 4097, 151_936])
def test_equal_logits_and_rows_that_are_nan_for_whole_waves(gpu, v):
    """Rows on which more candidates reach the top than the kernel holds in LDS (4096): all logits equal, and a row
    that is NaN outside the ids of one wave, so that the floor of the second pass is 0."""
    rng = np.random.default_rng(v)
    equal = np.full(v, 1.5, np.float32)
    waves = np.full(v, np.nan, np.float32)
    ids = np.arange(v)
    waves[ids % 1024 < 64] = _coarse(rng, int((ids % 1024 < 64).sum()))
    two = equal.copy()
    two[v // 2:] = np.float32(1.5) + np.float32(2.0 ** -20)    # two values, each held by half the row
    logits = np.stack([equal, waves, two])
    tokens = [v - 1, 5, 7]
    for n_top in (MAX_TOP, 1):
        out = _run(logits, tokens, None, n_top)
        for r in range(3):
            _check_row(out, r, logits[r], tokens[r], None, n_top, {})


def _raw(out):
    return {k: (None if t is None else t.view(torch.int32)) for k, t in out.items()}


def test_a_row_does_not_depend_on_the_call(gpu):
    rng = np.random.default_rng(11)
    v = 4097
    row, token, mask = _cases(rng, v)[0]
    others = _cases(np.random.default_rng(12), v)
    alone = _raw(_run(row[None], [token], mask[None], MAX_TOP))
    again = _raw(_run(row[None], [token], mask[None], MAX_TOP))
    for at in (0, 7):
        rows = [c[0] for c in others[:7]]
        rows[2] = np.full(v, np.nan, np.float32)                      # rows full of NaN beside it
        rows[5] = np.full(v, np.nan, np.float32)
        toks = [c[1] for c in others[:7]]
        masks = [c[2] for c in others[:7]]
        rows.insert(at, row), toks.insert(at, token), masks.insert(at, mask)
        many = _raw(_run(np.stack(rows), toks, np.stack(masks), MAX_TOP))
        for name, t in alone.items():
            assert torch.equal(t[0], many[name][at]), f"{name} of the row at position {at} of 8"
    for name, t in alone.items():
        assert torch.equal(t, again[name]), f"{name} on a second run"


def test_degenerate_rows(gpu):
    rng = np.random.default_rng(13)
    v = 1025
    cases = _cases(rng, v)
    logits = np.stack([c[0] for c in cases])
    tokens = [c[1] for c in cases]
    masks = np.stack([c[2] for c in cases])
    base = _raw(_run(logits, tokens, masks, MAX_TOP))
    logits2, tokens2, masks2 = logits.copy(), list(tokens), masks.copy()
    logits2[1] = np.nan                                # all NaN
    masks2[2] = False                                  # nothing allowed
    logits2[4, 77] = np.inf                            # a +inf maximum, the token a finite logit
    logits2[4, 78] = 0.25
    tokens2[4] = 78
    logits2[6, 9] = logits2[6, 500] = np.inf           # ... and the token ON a +inf maximum
    tokens2[6] = 500
    tokens2[0] = -1                                    # out of range on both sides
    tokens2[7] = v
    got = _run(logits2, tokens2, masks2, MAX_TOP)
    # row 1: no candidate
    assert float(got["lse_all"][1]) == -math.inf and float(got["lse_allowed"][1]) == -math.inf
    assert math.isnan(float(got["logprob"][1])) and int(got["rank"][1]) == 0
    assert got["top_id"][1].tolist() == [-1] * MAX_TOP and bool(torch.isnan(got["top_logprob"][1]).all())
    # row 2: an empty allowed set
    assert float(got["lse_allowed"][2]) == -math.inf and math.isfinite(float(got["lse_all"][2]))
    # row 4: +inf maximum, finite token
    assert float(got["lse_all"][4]) == math.inf and float(got["logprob"][4]) == -math.inf
    assert int(got["top_id"][4, 0]) == 77 and math.isnan(float(got["top_logprob"][4, 0]))
    assert float(got["top_logprob"][4, 1]) == -math.inf
    # row 6: the token on one of two +inf maxima: inf - inf, and still a rank
    assert math.isnan(float(got["logprob"][6])) and int(got["rank"][6]) == 1
    assert got["top_id"][6, :2].tolist() == [9, 500]
    # rows 0 and 7: ids outside the row
    for r in (0, 7):
        assert math.isnan(float(got["logprob"][r])) and int(got["rank"][r]) == 0
    for r in range(8):
        _check_row(got, r, logits2[r], tokens2[r], masks2[r], MAX_TOP, {})
    raw = _raw(got)
    for r in (3, 5):                                   # the rows nothing was done to
        for name in base:
            assert torch.equal(base[name][r], raw[name][r]), f"{name} of untouched row {r}"
    for name in ("lse_all", "lse_allowed", "top_id", "top_logprob"):    # rows whose token alone changed
        for r in (0, 7):
            assert torch.equal(base[name][r], raw[name][r]), f"{name} of row {r}"


def test_refusals_leave_the_outputs_alone(gpu):
    v, n, n_top = 100, 2, 4
    lg = torch.randn(n, v, device=DEV)
    tok = torch.zeros(n, dtype=torch.int32, device=DEV)
    bits = torch.full((n, 4), -1, dtype=torch.int32, device=DEV)
    bufs = {"logprob": torch.full((n + 1,), FLOAT_FILL, device=DEV), "lse_all": torch.full((n + 1,), FLOAT_FILL, device=DEV),
            "lse_allowed": torch.full((n + 1,), FLOAT_FILL, device=DEV),
            "rank": torch.full((n + 1,), INT_FILL, dtype=torch.int32, device=DEV),
            "top_id": torch.full((n * n_top + 1,), INT_FILL, dtype=torch.int32, device=DEV),
            "top_logprob": torch.full((n * n_top + 1,), FLOAT_FILL, device=DEV)}
    before = {k: t.clone() for k, t in bufs.items()}
    ptr = lambda t, off=0: None if t is None else ctypes.c_void_p(t.data_ptr() + off)   # noqa: E731
    ok = dict(logits=ptr(lg), vocab=v, bits=ptr(bits), token=ptr(tok), logprob=ptr(bufs["logprob"]),
              lse_all=ptr(bufs["lse_all"]), lse_allowed=ptr(bufs["lse_allowed"]), rank=ptr(bufs["rank"]),
              top_id=ptr(bufs["top_id"]), top_logprob=ptr(bufs["top_logprob"]), n_top=n_top, n_rows=n)

    def call(**change):
        a = dict(ok, **change)
        return gpu.crag_enc_logprobs(a["logits"], a["vocab"], a["bits"], a["token"], a["logprob"], a["lse_all"],
                                     a["lse_allowed"], a["rank"], a["top_id"], a["top_logprob"], a["n_top"], a["n_rows"],
                                     None)

    refusals = [dict(logits=None), dict(token=None), dict(logprob=None), dict(n_rows=0), dict(n_rows=9), dict(n_rows=-1),
                dict(vocab=0), dict(vocab=-5), dict(vocab=2 ** 31), dict(n_top=-1), dict(n_top=17), dict(n_top=3, vocab=2),
                dict(top_id=None), dict(top_logprob=None)]
    refusals += [{name: ptr(t, 2)} for name, t in (("logits", lg), ("bits", bits), ("token", tok))]
    refusals += [{name: ptr(t, 2)} for name, t in bufs.items()]
    for change in refusals:
        assert call(**change) == -1, f"{sorted(change)} was not refused with CRAG_EINVAL"
    torch.cuda.synchronize()
    for name, t in bufs.items():
        assert torch.equal(t, before[name]), f"a refused call wrote {name}"
    assert call() == 0 and call(n_top=0, top_id=None, top_logprob=None) == 0      # and the call itself is a good one
    torch.cuda.synchronize()
    assert not torch.equal(bufs["logprob"][:n], before["logprob"][:n])
    assert float(bufs["logprob"][n]) == FLOAT_FILL and int(bufs["top_id"][n * n_top]) == INT_FILL   # nothing behind the end
