"""crag_enc_adjust_logits against the host rule (penalties.adjust_host), BIT FOR BIT on the adjusted rows (int32 view; NaN
positions compared as masks, their payloads left out) and on the token: the sizes at which the kernel's loops end, every
clause alone and all together, the roundings of steps a and b on > 100 000 random operands, specials and ties, the
independence of a row from its neighbours, and every refusal of the entry through ops.  Inputs avoid subnormals."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cadence_rag_amd import _native
from cadence_rag_amd.penalties import PenaltyParams, adjust_host, exempt_words

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
INF = math.inf
ALL = PenaltyParams(repetition_penalty=1.3, presence_penalty=0.6, frequency_penalty=0.4, no_repeat_ngram=3)


def _run(logits: np.ndarray, log: np.ndarray, rows, exempt=None, inplace=False, shift=0):
    """rows: one (log row, prompt_len, total_len, params, bias list) per row of logits -> (out, token) from the kernel.
    shift: out begins that many floats behind a 16-byte boundary, so its rows are misaligned otherwise than the logits'."""
    from cadence_rag_amd.encoder import ops
    n, vocab = logits.shape
    src = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).to(DEV)
    out = src if inplace else torch.full((n * vocab + shift,), 123.0, device=DEV)[shift:].view(n, vocab)
    token = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    ws = ops.adjust_workspace(n, vocab, DEV)
    ws.fill_(0xA5)                                     # the kernel zeroes its slice itself
    bias = {}
    if any(r[4] for r in rows):
        flat = [e for r in rows for e in r[4]]
        bias = dict(bias_ids=torch.tensor([t for t, _ in flat], dtype=torch.int32).to(DEV),
                    bias_values=torch.tensor([b for _, b in flat], dtype=torch.float32).to(DEV),
                    bias_offsets=np.concatenate([[0], np.cumsum([len(r[4]) for r in rows])]).tolist())
    bits = None if exempt is None else torch.from_numpy(exempt_words(exempt, vocab).view(np.int32)).to(DEV)
    ops.adjust_logits(src, out, torch.from_numpy(np.ascontiguousarray(log, dtype=np.int32)).to(DEV),
                      [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], token, ws,
                      exempt_bits=bits, **bias)
    torch.cuda.synchronize()
    return out.cpu().numpy(), token.cpu().numpy()


def _same_bits(got: np.ndarray, want: np.ndarray, what: str) -> None:
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions"
    differ = np.nonzero((got.view(np.int32) != want.view(np.int32)) & ~nan)[0]
    assert differ.size == 0, f"{what}: {differ.size} ids differ, first {differ[0]}: {got[differ[0]]!r} for {want[differ[0]]!r}"


def _check(logits, log, rows, exempt=None, inplace=False, what=""):
    got, token = _run(logits, log, rows, exempt, inplace)
    for r, (log_row, prompt_len, total, params, bias) in enumerate(rows):
        want, want_token = adjust_host(logits[r], log[log_row], prompt_len, params, exempt=exempt, bias=bias, total=total)
        _same_bits(got[r], want, f"{what} row {r}")
        assert int(token[r]) == want_token, f"{what} row {r}: token {int(token[r])} for {want_token}"
    return got, token


def _logits(rng, n, vocab):
    x = (rng.standard_normal((n, vocab)) * 4).astype(np.float32)
    x[np.abs(x) < 1e-3] = 0.5            # far from subnormal results
    return x


LENGTHS = [0, 1, 2, 1023, 1024, 1025, 8192, 8192]


def _size_case(rng, vocab):
    """Eight rows over a log of 8192 columns: the history lengths at which the scatter loop's trips change, prompt_len 0,
    in between and equal to total_len, ids just outside the vocabulary, and (last row) one id 8191 times."""
    log = rng.integers(-2, vocab + 2, (8, 8192)).astype(np.int32)
    log[7, :] = vocab // 2
    log[7, 5000] = 0
    prompts = [0, 1, 1, 500, 1024, 0, 4000, 0]
    rows = [(r, prompts[r], LENGTHS[r], ALL, []) for r in range(8)]
    return _logits(rng, 8, vocab), log, rows


@pytest.mark.parametrize("vocab", [1, 33, 384, 4099])
def test_sizes(gpu, vocab):
    rng = np.random.default_rng(vocab)
    _check(*_size_case(rng, vocab), what=f"vocab {vocab}")


def test_the_4b_vocabulary_with_eight_rows(gpu):
    rng = np.random.default_rng(11)
    logits, log, rows = _size_case(rng, 151_936)
    log[2:7] = rng.integers(0, 300, (5, 8192))          # few distinct ids: counts and n-gram matches happen
    bias = [(int(t), float(b)) for t, b in zip(np.sort(rng.choice(151_936, 256, replace=False)), rng.uniform(-100, 100, 256))]
    rows[6] = rows[6][:4] + (bias,)
    _check(logits, log, rows, exempt=rng.choice(151_936, 2000, replace=False), what="vocab 151936")


def _repeating_log(rng, vocab, stride=256):
    """A log whose rows repeat a phrase of 11 ids: n-grams of every size up to 8 occur again."""
    phrase = rng.integers(0, vocab, 11)
    log = np.tile(phrase, stride // 11 + 1)[:stride][None, :].repeat(2, 0).astype(np.int32)
    log[1, ::7] = rng.integers(0, vocab, log[1, ::7].size)      # row 1: the phrase with holes
    return log


CLAUSES = {
    "repetition": PenaltyParams(repetition_penalty=1.3),
    "reward": PenaltyParams(repetition_penalty=0.7),
    "frequency": PenaltyParams(frequency_penalty=0.37),
    "presence": PenaltyParams(presence_penalty=-0.81),
    "ngram2": PenaltyParams(no_repeat_ngram=2),
    "ngram3": PenaltyParams(no_repeat_ngram=3),
    "ngram8": PenaltyParams(no_repeat_ngram=8),
    "neutral": PenaltyParams(),
    "all": PenaltyParams(repetition_penalty=1.7, presence_penalty=1.1, frequency_penalty=-0.3, no_repeat_ngram=2),
}


@pytest.mark.parametrize("clause", list(CLAUSES))
def test_each_clause_alone_and_all_together(gpu, clause):
    rng = np.random.default_rng(5)
    vocab = 4099
    log = _repeating_log(rng, vocab)
    logits = _logits(rng, 4, vocab)
    p = CLAUSES[clause]
    rows = [(0, 40, 256, p, []), (1, 0, 200, p, []), (0, 100, 100, p, []), (1, 13, 21, p, [])]
    got, _ = _check(logits, log, rows, what=clause)
    if clause.startswith("ngram") or clause == "all":
        assert (got[0] == -INF).sum() >= 1 and not (got[2] == -INF).any()      # a ban happened; none without output
    if clause == "neutral":
        assert np.array_equal(got.view(np.int32), logits.view(np.int32))
    # the same with exempt ids, and with bias lists of 0, 1 and 256 entries, -inf among them
    exempt = np.unique(np.concatenate([log[0, :64], rng.choice(vocab, 50)]))
    ids = np.sort(rng.choice(vocab, 256, replace=False))
    ids[:4] = np.sort(log[0, :11])[:4] if len(set(log[0, :11])) == 11 else ids[:4]
    ids = np.unique(ids)
    values = rng.uniform(-100, 100, ids.size).astype(np.float32)
    values[::5] = -INF
    big = list(zip(ids.tolist(), values.tolist()))
    rows = [(0, 40, 256, p, []), (1, 0, 200, p, big[7:8]), (0, 100, 100, p, big), (1, 13, 21, p, big[:3])]
    _check(logits, log, rows, exempt=exempt, what=clause + " + exempt + bias")
    _check(logits, log, rows, what=clause + " + bias")


def test_rounding_of_the_division_and_of_the_three_step_subtraction(gpu):
    """8 x 16384 random (l, rp, frequency, c, presence): an approximate division, or f * c - fused into the subtraction,
    differs from the host rule in a share of them."""
    rng = np.random.default_rng(23)
    vocab, n = 16384, 8
    logits = _logits(rng, n, vocab) * np.float32(3.7)
    counts = rng.integers(0, 6, (n, vocab))
    counts[:, ::3] = rng.integers(1, 40, counts[:, ::3].shape)
    stride = int(counts.sum(1).max()) + 8
    log = np.full((n, stride), -1, dtype=np.int32)
    rows = []
    for r, (rp, fr, pr) in enumerate([(1.3, 0.1, 0.3), (0.7, 1.9, -0.7), (1.3, -0.123, 1.999), (0.7, 0.3, 0.1),
                                      (3.3333, 0.7, 0.0), (1.0, 0.9, 0.45), (1.1, 0.0, 0.0), (9.9, 2.0, 2.0)]):
        ids = np.repeat(np.arange(vocab), counts[r])
        rng.shuffle(ids)
        log[r, :ids.size] = ids
        rows.append((r, 0, int(ids.size), PenaltyParams(repetition_penalty=rp, frequency_penalty=fr, presence_penalty=pr), []))
    _check(logits, log, rows, what="rounding")
    # the test can see a fused multiply-add: an fp64 product inside the subtraction differs on these operands
    l, c = logits[0].astype(np.float64), counts[0].astype(np.float64)
    base = np.where(l > 0, (logits[0] / np.float32(1.3)), logits[0] * np.float32(1.3)).astype(np.float32)
    fused = (base.astype(np.float64) - np.float64(np.float32(0.1)) * c).astype(np.float32)
    plain = (base - (np.float32(0.1) * counts[0].astype(np.float32)).astype(np.float32)).astype(np.float32)
    assert (fused != plain).sum() > 100


def test_specials_and_ties(gpu):
    log = np.array([[0, 1, 2, 3, 4, 5, 6, 1, 9, 9, 9, 0]], dtype=np.int32)
    row = np.array([2.6, -2.6, 0.0, -0.0, INF, -INF, math.nan, 1.0, 3.0, 6.0, 3.0, 1.0], dtype=np.float32)
    logits = np.stack([row, row, row, np.full(12, math.nan, dtype=np.float32), np.full(12, -INF, dtype=np.float32), row])
    rows = [(0, 7, 7, PenaltyParams(repetition_penalty=1.3), []),                       # the sign branch at 0, -0, inf, NaN
            (0, 0, 11, PenaltyParams(presence_penalty=1.0, frequency_penalty=1.0), []),  # 9 three times: (6 - 3) - 1
            (0, 7, 11, PenaltyParams(repetition_penalty=2.0), []),                       # 6 / 2 = 3 ties ids 8 and 10
            (0, 0, 12, ALL, []),                                                           # all NaN: -1
            (0, 0, 12, ALL, [(3, 5.0)]),                                                   # all -inf: the lowest id
            (0, 0, 0, PenaltyParams(logit_bias={}), [(4, -INF), (9, -3.0)])]               # inf - inf = NaN leaves the row
    got, token = _check(logits, log, rows, what="specials")
    assert np.signbit(got[0, 3]) and not np.signbit(got[0, 2]) and got[0, 4] == INF
    assert token.tolist() == [4, 4, 4, -1, 0, 8] and math.isnan(got[5, 4])
    assert got[2, 8] == got[2, 9] == got[2, 10] == 3.0


def test_a_row_does_not_depend_on_its_neighbours(gpu):
    rng = np.random.default_rng(31)
    vocab = 4099
    log = rng.integers(0, 64, (3, 700)).astype(np.int32)
    logits = _logits(rng, 8, vocab)
    params = [PenaltyParams(repetition_penalty=1.0 + 0.2 * r, presence_penalty=0.25 * r - 1, frequency_penalty=0.1 * r,
                            no_repeat_ngram=(0, 2, 3, 4, 5, 6, 7, 8)[r]) for r in range(8)]
    bias = [[], [(5, 1.0)], [], [(1, -INF), (70, 2.0)], [], [], [(4098, -1.0)], []]
    # rows 2 and 3 (and 5, 6, 7) share a log row at different lengths: a sequence's rows under speculation
    rows = [(0, 10, 700, params[0], bias[0]), (1, 0, 64, params[1], bias[1]), (2, 100, 300, params[2], bias[2]),
            (2, 100, 301, params[3], bias[3]), (1, 64, 64, params[4], bias[4]), (0, 10, 11, params[5], bias[5]),
            (0, 10, 12, params[6], bias[6]), (0, 10, 13, params[7], bias[7])]
    exempt = rng.choice(64, 9, replace=False)
    got, token = _check(logits, log, rows, exempt=exempt, what="eight rows")
    for r in (0, 3, 7):
        alone, alone_token = _run(logits[r:r + 1], log, [rows[r]], exempt)
        assert np.array_equal(alone[0].view(np.int32), got[r].view(np.int32)) and int(alone_token[0]) == int(token[r])
    same, same_token = _run(logits, log, rows, exempt, inplace=True)
    assert np.array_equal(same.view(np.int32), got.view(np.int32)) and np.array_equal(same_token, token)
    for shift in (1, 2, 3):     # out misaligned otherwise than logits: the 4-byte stores
        moved, moved_token = _run(logits, log, rows, exempt, shift=shift)
        assert np.array_equal(moved.view(np.int32), got.view(np.int32)) and np.array_equal(moved_token, token)
    again, again_token = _run(logits, log, rows, exempt)
    assert np.array_equal(again.view(np.int32), got.view(np.int32)) and np.array_equal(again_token, token)


def test_refusals_through_ops(gpu):
    from cadence_rag_amd.encoder import ops
    vocab = 100
    logits = torch.zeros(2, vocab, dtype=torch.float32, device=DEV)
    out = torch.empty_like(logits)
    log = torch.zeros(2, 16, dtype=torch.int32, device=DEV)
    token = torch.empty(2, dtype=torch.int32, device=DEV)
    ws = ops.adjust_workspace(2, vocab, DEV)
    ok = dict(logits=logits, out=out, history=log, history_rows=[0, 1], prompt_lens=[1, 2], total_lens=[3, 16],
              params=PenaltyParams(), token=token, workspace=ws)
    ops.adjust_logits(**ok)
    ids = torch.tensor([3, 5, 9], dtype=torch.int32, device=DEV)
    vals = torch.tensor([1.0, -INF, 2.0], dtype=torch.float32, device=DEV)
    ops.adjust_logits(**ok, bias_ids=ids, bias_values=vals, bias_offsets=[0, 1, 3])
    torch.cuda.synchronize()

    def bad(code_text, **kw):
        with pytest.raises(_native.NativeLibraryError, match=code_text):
            ops.adjust_logits(**dict(ok, **kw))

    odd = lambda **kw: [SimpleNamespace(**dict(dict(repetition_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0,   # noqa: E731
                                                    no_repeat_ngram=0), **kw)), PenaltyParams()]
    einval = "code -1"
    bad(einval, history_rows=[0, 2]); bad(einval, history_rows=[-1, 0])
    bad(einval, prompt_lens=[4, 2]); bad(einval, prompt_lens=[-1, 2])
    bad(einval, total_lens=[3, 17]); bad(einval, total_lens=[-1, 16], prompt_lens=[-1, 2])
    for kw in (dict(repetition_penalty=0.05), dict(repetition_penalty=10.5), dict(repetition_penalty=math.nan),
               dict(frequency_penalty=2.5), dict(frequency_penalty=math.nan), dict(presence_penalty=-2.5),
               dict(no_repeat_ngram=1), dict(no_repeat_ngram=9), dict(no_repeat_ngram=-3)):
        bad(einval, params=odd(**kw))
    bad(einval, bias_ids=ids, bias_values=vals, bias_offsets=[1, 1, 3])          # not from 0
    bad(einval, bias_ids=ids, bias_values=vals, bias_offsets=[0, 2, 1])          # falling
    unordered = torch.tensor([3, 9, 5], dtype=torch.int32, device=DEV)
    bad("ascending", bias_ids=unordered, bias_values=vals, bias_offsets=[0, 0, 3])
    twice = torch.tensor([3, 5, 5], dtype=torch.int32, device=DEV)
    bad("ascending", bias_ids=twice, bias_values=vals, bias_offsets=[0, 1, 3])
    outside = torch.tensor([3, 5, 100], dtype=torch.int32, device=DEV)
    bad("ascending", bias_ids=outside, bias_values=vals, bias_offsets=[0, 1, 3])
    many = torch.arange(257, dtype=torch.int32, device=DEV)
    big = torch.zeros(2, 300, dtype=torch.float32, device=DEV)
    bad(einval, logits=big, out=torch.empty_like(big), workspace=ops.adjust_workspace(2, 300, DEV), bias_ids=many,
        bias_values=torch.zeros(257, device=DEV), bias_offsets=[0, 257, 257])    # a slice longer than 256
    bad("aligned", workspace=torch.empty(ws.numel() + 4, dtype=torch.uint8, device=DEV)[1:])
    bad("code -5", workspace=ws[:ws.numel() - 4])                                # CRAG_E2BIG
    nine = torch.zeros(9, vocab, dtype=torch.float32, device=DEV)
    with pytest.raises(_native.NativeLibraryError, match="n_rows"):
        ops.adjust_logits(nine, torch.empty_like(nine), log, [0] * 9, [0] * 9, [0] * 9, PenaltyParams(),
                          torch.empty(9, dtype=torch.int32, device=DEV), ws)
    with pytest.raises(ValueError):
        ops.adjust_workspace(9, vocab, DEV)
    with pytest.raises(ValueError):
        ops.adjust_workspace(1, 0, DEV)
    for kw in (dict(logits=logits.double()), dict(out=out[:1]), dict(history=log.long()), dict(history_rows=[0]),
               dict(bias_ids=ids), dict(exempt_bits=torch.zeros(3, dtype=torch.int32, device=DEV)),
               dict(bias_ids=ids, bias_values=vals, bias_offsets=[0, 1])):
        with pytest.raises(ValueError):
            ops.adjust_logits(**dict(ok, **kw))
    assert _native.CRAG_E2BIG == -5
