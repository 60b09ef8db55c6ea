"""crag_enc_sample on the paths random rows do not reach, against sampling.sample_host (fp64).  The cases and what each is
for: tests/sample_probes.py; that each takes the path it is meant for, that the host is sure wherever a token is compared
and that each family of cases has teeth: tests/test_sample_probes_host.py.

Every case runs as a row alone and as one of 8 mixed rows of one call, in both of its forms: the ids that are no
candidates hold -inf / NaN, or hold logits that would win and are banned through allowed_bits.

  selection     top_p == 1: the kept count and the bits of the lowest kept logit are the host's, the token is an allowed
                id at or above the cut, and the host's own where its two best keys are more than EPS apart.  Rows that
                fill LDS exactly and rows one id past it, rows far past it (one level-0 bin, a tied block of 5000), k-th
                keys on the first and last digits of the lower radix levels, thresholds on denormals and on the zeros of
                both signs, the real vocabulary with top_k past the capacity, temperature 0.01 and 100, a row holding
                the largest float of both signs.
  sure          top-p behind a top-k that stayed on the row, and top-p that never compacts: compared by the rule of
                test_sample_gpu.py's draw test (the host's token is the same under top_p (1 -+ DELTA) and its gap is
                above EPS; then the token is equal and the kept count within the host's band); at least 98 % compared.
  noise         the draws at the ends of the uniform and at the switch between gumbel()'s two formulas, planted on the
                (step, id) pairs of sample_probes.NOISE; every case is compared.
  seeds         seeds with a high half, steps and streams with high bits; at least 98 % compared."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import sample_probes as sp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
FORMS = ("inf", "bits")


def _pack(allowed: np.ndarray) -> torch.Tensor:
    """bool [n, V] -> int32 [n, ceil(V / 32)], bit t % 32 of word t / 32."""
    n, v = allowed.shape
    padded = np.zeros((n, (v + 31) // 32 * 32), np.uint8)
    padded[:, :v] = allowed
    words = np.packbits(padded, axis=1, bitorder="little").view(np.uint32)
    return torch.from_numpy(words.view(np.int32).copy()).to(DEV)


def _sample(logits: np.ndarray, params, step, streams, allowed=None):
    """One call: (tokens, kept counts, the bits of cut), lists of n."""
    from cadence_rag_amd.encoder import ops
    n = logits.shape[0]
    lg = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).to(DEV)
    token = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    kept = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    cut = torch.full((n,), 123.0, dtype=torch.float32, device=DEV)
    ops.sample(lg, params, step, streams, token, allowed_bits=None if allowed is None else _pack(allowed), kept=kept,
               cut=cut)
    return token.cpu().tolist(), kept.cpu().tolist(), cut.cpu().numpy().view(np.uint32).tolist()


def _bits(x: float) -> int:
    return int(np.float32(x).view(np.uint32))


def _run(block: str, rows: int, form: str):
    """Every row of every call of the block: (case, logits, allowed or None, token, kept, bits of cut)."""
    for call in sp.calls_of(block, rows):
        built = [c.row(form) for c in call]
        x = np.stack([b[0] for b in built])
        allowed = None if form == "inf" else np.stack([b[1] for b in built])
        token, kept, cut = _sample(x, [c.params for c in call], call[0].step, [c.stream for c in call], allowed=allowed)
        for r, case in enumerate(call):
            yield case, x[r], None if allowed is None else allowed[r], token[r], kept[r], cut[r]


def _check_exact(case, row, allowed, token, kept, cut):
    ref = case.reference()
    assert (kept, cut) == (ref.kept, _bits(ref.cut)), (case.name, kept, np.uint32(cut).view(np.float32), ref)
    assert 0 <= token < case.v and (allowed is None or allowed[token]) and row[token] >= ref.cut, (case.name, token, ref)
    if ref.gap > sp.EPS:
        assert token == ref.token, (case.name, token, ref)
    return ref.gap > sp.EPS


def _check_sure(case, token, kept) -> bool:
    ref = case.reference()
    if not (ref.stable and ref.gap > sp.EPS):
        return False
    assert token == ref.token, (case.name, token, ref)
    assert ref.kept_lo <= kept <= ref.kept_hi, (case.name, kept, ref)
    return True


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("rows", [1, 8])
@pytest.mark.parametrize("block", sp.EXACT_BLOCKS)
def test_selection_is_exact(gpu, block, rows, form):
    exact = tokens = sure = compared = 0
    for case, row, allowed, token, kept, cut in _run(block, rows, form):
        if case.sure:
            sure += 1
            compared += _check_sure(case, token, kept)
        else:
            exact += 1
            tokens += _check_exact(case, row, allowed, token, kept, cut)
    print(f"{block}, {rows} rows, {form}: {exact} rows exact, {tokens} tokens compared; top-p: {compared} of {sure} compared")
    assert exact >= len([c for c in sp.cases_of(block) if not c.sure]) and compared >= 0.98 * sure


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("rows", [1, 8])
def test_top_p_off_the_row_equals_the_host_where_the_host_is_sure(gpu, rows, form):
    compared = total = 0
    for case, _, allowed, token, kept, _ in _run("sure", rows, form):
        total += 1
        compared += _check_sure(case, token, kept)
        assert 0 <= token < case.v and (allowed is None or allowed[token])
    print(f"sure, {rows} rows, {form}: {compared} of {total} cases compared")
    assert total >= len(sp.cases_of("sure")) and compared >= 0.98 * total, (compared, total)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("rows", [1, 8])
def test_noise_tails_do_not_lose_the_winner(gpu, rows, form):
    total = 0
    for case, row, allowed, token, kept, cut in _run("noise", rows, form):
        ref = case.reference()
        total += 1
        assert ref.gap > sp.EPS and token == ref.token == case.token, (case.name, token, ref)
        assert (kept, cut) == (ref.kept, _bits(ref.cut)), (case.name, kept, ref)
    print(f"noise, {rows} rows, {form}: {total} of {total} cases compared")
    assert total >= len(sp.cases_of("noise"))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("rows", [1, 8])
def test_the_whole_seed_and_the_whole_counters_reach_the_generator(gpu, rows, form):
    compared = total = 0
    got = {}
    for case, row, allowed, token, kept, cut in _run("seeds", rows, form):
        total += 1
        compared += _check_exact(case, row, allowed, token, kept, cut)
        got[case.name] = token
    print(f"seeds, {rows} rows, {form}: {compared} of {total} cases compared")
    assert total >= len(sp.cases_of("seeds")) and compared >= 0.98 * total, (compared, total)
    for name, token in got.items():           # 5 and 5 + 2^32 draw differently on one row, as the host says they do
        if name.startswith("seed 0x5 "):
            assert token != got[name.replace("seed 0x5 ", f"seed {5 + (1 << 32):#x} ")], name
