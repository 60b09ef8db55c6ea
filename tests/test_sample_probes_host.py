"""What tests/test_sample_probes_gpu.py rests on, proven without a GPU (tests/sample_probes.py):

  * fkey_host is the order of the floats, with -0 and +0 one key;
  * every NOISE entry draws the k it is listed under, and the Gumbel values at the ends and at the formula switch;
  * for every case the GPU file runs: both forms hold the same candidates; path_of names the path the case is meant for
    (compaction or not, at which selection, which level decides, n_ge on its side of the capacity); where the token is
    compared the host is stable with a gap above EPS; where kept is compared exactly, kept_lo == kept_hi;
  * teeth -- a numpy model of the selection, or the host rule, with one fault applied, changes the answer of the cases
    built against that fault: the level-0 set truncated at the capacity, the lowest radix level dropped, the keys of
    negative floats not inverted, seed_hi zeroed, step and stream taken mod 2^16, the noise of a planted id 0.02 lower.

Two of the teeth cannot bite everywhere, and the assertions say where: a top_k whose k-th key has the last digit 0 keeps
the whole of a low_level_only row, with or without its lowest level; and a truncated set still holds top_k ids while
top_k is at most the capacity, so there the cut moves (the two largest values sit on the highest ids, the first a
truncation in id order loses) and the count only beyond it."""
from __future__ import annotations

import numpy as np
import pytest

import sample_probes as sp
from cadence_rag_amd.sampling import SamplingParams, philox_uniform_host, sample_host


# ---- the key --------------------------------------------------------------------------------------------------------------
def test_fkey_host_is_strictly_monotone_and_folds_the_zeros():
    mx, tiny, dmin = np.float32(sp.FLT_MAX), np.float32(np.finfo(np.float32).tiny), np.float32(sp.DENORM_MIN)
    below = lambda x: np.nextafter(np.float32(x), np.float32(-np.inf))     # noqa: E731
    above = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))      # noqa: E731
    rng = np.random.default_rng(0)
    special = [-np.inf, -mx, above(-mx), -1.0, -tiny, below(-tiny), above(-tiny), -dmin, below(-dmin), 0.0, dmin, above(dmin),
               below(tiny), tiny, above(tiny), 1.0, below(1.0), above(1.0), below(mx), mx, np.inf]
    random = sp.from_bits(rng.integers(0, 1 << 32, 20_000, dtype=np.uint32))
    x = np.unique(np.concatenate([np.asarray(special, np.float32), random[~np.isnan(random)]]))   # ascending, -0 == 0 once
    keys = sp.fkey_host(x).astype(np.int64)
    assert (np.diff(keys) > 0).all()
    assert sp.fkey_host(np.float32(-0.0))[0] == sp.fkey_host(np.float32(0.0))[0] == 0x80000000
    assert sp.fkey_host(-dmin)[0] == 0x7FFFFFFE and sp.fkey_host(dmin)[0] == 0x80000001
    # the fault the teeth use really is another order
    assert sp.fkey_without_inversion(np.float32(-2.0))[0] == sp.fkey_host(np.float32(2.0))[0]


# ---- the noise ------------------------------------------------------------------------------------------------------------
def test_every_noise_entry_draws_its_k():
    for kind, entries in sp.NOISE.items():
        lo, hi = sp.NOISE_K[kind]
        for step, token in entries:
            u = philox_uniform_host(sp.NOISE_SEED, step, 0, [token])[0]
            k = int(round(u * 2.0 ** 24 - 0.5))
            assert lo <= k <= hi, (kind, step, token, hex(k))
            assert k == int(sp.draw_k(sp.NOISE_SEED, step, 0, [token])[0]) and token < sp.VOCAB
    step, token = sp.LOWEST_U
    u = philox_uniform_host(sp.NOISE_SEED, step, 0, np.arange(sp.VOCAB))
    assert int(np.argmin(u)) == token and abs(u[token] - 6.7e-6) < 1e-7
    assert abs(-np.log(-np.log(u[token])) + 2.4776) < 1e-4
    assert np.array_equal(-np.log(-np.log(u)), sp.step_gumbel(step))


def test_gumbel_values_at_the_ends_and_at_the_switch():
    g = sp.gumbel_of_k([0xFFFFFF, 0, (1 << 23) - 1, 1 << 23])
    assert abs(g[0] - (25 * np.log(2.0) + 2.0 ** -26)) < 1e-6   # -ln(-ln(1 - 2^-25)): 17.3287
    assert abs(g[1] + np.log(25 * np.log(2.0))) < 1e-6          # -ln(-ln 2^-25): -2.852
    half = -np.log(np.log(2.0))                               # 0.366513, u = 1/2
    assert g[2] < half < g[3] and abs(g[2] - half) < 1e-6 and abs(g[3] - half) < 1e-6
    assert abs(half - 0.3665) < 1e-4 and abs(g[0] - 17.3287) < 1e-4 and abs(g[1] + 2.852) < 1e-3


# ---- every case of the GPU file ---------------------------------------------------------------------------------------------
def _way(sel):
    if sel is None:
        return None
    return "held" if sel.from_lds else "lds" if sel.compacts else "row"


@pytest.mark.parametrize("block", sp.BLOCKS)
def test_both_forms_hold_the_same_candidates(block):
    for case in sp.cases_of(block):
        values, ids = case.layout()
        plain, none = case.row("inf")
        poisoned, allowed = case.row("bits")
        assert none is None and plain.size == poisoned.size == allowed.size == case.v
        cand = ~np.isnan(plain) & (plain != -np.inf)
        assert np.array_equal(np.nonzero(cand)[0], np.sort(ids[np.isfinite(values) | (values == np.inf)]))
        assert np.array_equal(cand, allowed & ~np.isnan(poisoned) & (poisoned != -np.inf))
        assert np.array_equal(plain[cand].view(np.uint32), poisoned[cand].view(np.uint32))
        off = ~allowed
        if off.any() and block != "noise":          # ignoring the bits would change the maximum, hence every answer
            assert np.nanmax(poisoned[off]) == np.float32(sp.FLT_MAX) > plain[cand].max() or case.name.count("extremes")


@pytest.mark.parametrize("block", sp.BLOCKS)
def test_each_case_takes_the_path_it_is_meant_for(block):
    for case in sp.cases_of(block):
        row, _ = case.row("inf")
        path = sp.path_of(row, case.params)
        where = (case.name, path)
        if case.count is not None or block in ("capacity", "past", "levels", "zero"):
            assert _way(path.count) == case.count, where
        if case.weight is not None or block == "sure":
            assert path.weight is not None and (case.weight is None or _way(path.weight) == case.weight), where
        if case.count == "lds":
            assert path.count.n_ge <= sp.CAP, where
        if case.count == "row":
            assert path.count.n_ge > sp.CAP, where
        if case.weight == "row":
            assert path.weight.n_ge > sp.CAP, where
        if case.n_ge is not None:
            assert path.count.n_ge == case.n_ge, where
        if case.occupied is not None:
            assert all(w is None or w == o for w, o in zip(case.occupied, path.count.occupied)), where
        for level, d in case.digits.items():
            assert sp.digit(path.count.key, level) == d, where
        if block in ("noise", "seeds"):
            assert path == (None, None) or case.params.top_k == 50, where


def test_the_blocks_reach_every_path_the_issue_names():
    """Not only case by case: together the cases hold each path at least once."""
    ways = set()
    for block in sp.BLOCKS:
        for case in sp.cases_of(block):
            if block in ("noise", "seeds"):
                continue
            path = sp.path_of(case.row("inf")[0], case.params)
            ways.add((_way(path.count), _way(path.weight)))
    assert {("lds", None), ("row", None), ("row", "lds"), ("row", "row"), (None, "row")} <= ways, ways
    edge = {c.n_ge for c in sp.cases_of("capacity")}
    assert edge == {sp.CAP, sp.CAP + 1}
    # a top-p behind an uncompacted top-k compacts above the floor: its level-0 bin lies above the k-th key's
    above = [c.name for c in sp.cases_of("sure")
             for p in [sp.path_of(c.row("inf")[0], c.params)] if p.count and p.weight.compacts and p.weight.bin0 > p.count.bin0]
    assert above, "no top-p compaction with low > floor_key"
    digits = {(lvl, d) for c in sp.cases_of("levels") for lvl, d in c.digits.items()}
    assert digits == {(2, 0), (2, 1), (2, 1022), (2, 1023), (1, 0), (1, 1), (1, 2046), (1, 2047)}


@pytest.mark.parametrize("block", sp.EXACT_BLOCKS)
def test_exact_cases_have_one_kept_count(block):
    for case in sp.cases_of(block):
        ref = case.reference()
        if case.sure:
            continue
        assert case.params.top_p == 1.0 and ref.kept_lo == ref.kept == ref.kept_hi and ref.stable, case.name
        assert ref.token >= 0 and np.isfinite(ref.cut), case.name


def test_zeros_of_both_signs_stay_together_at_scale():
    case = sp.CASES["around_zero zero mp0.0"]
    values, _ = case.layout()
    zeros = int((values == 0).sum())
    ref = case.reference()
    assert zeros > sp.CAP and int(np.signbit(values[values == 0]).sum()) == zeros // 2
    assert ref.cut == 0.0 and ref.kept == int((values >= 0).sum())
    for name, cut in (("smallest denormal", sp.DENORM_MIN), ("smallest negative denormal", -sp.DENORM_MIN),
                      ("negative denormal", sp.NEG_DENORM)):
        ref = sp.CASES[f"around_zero {name} mp0.0"].reference()
        assert ref.cut == cut and ref.kept == int((values >= np.float32(cut)).sum()), name


def _sure(ref) -> bool:
    return ref.stable and ref.gap > sp.EPS


@pytest.mark.parametrize("block", ["sure", "seeds", "temperature"])
def test_the_host_alone_is_sure_of_at_least_98_percent(block):
    cases = [c for c in sp.cases_of(block) if c.sure]
    compared = sum(_sure(c.reference()) for c in cases)
    assert len(cases) >= 4 and compared >= 0.98 * len(cases), (compared, len(cases))
    if block == "sure":                       # the boundary of the tied rows falls inside the block of 5000
        for c in cases:
            if "tied" in c.name:
                ref = c.reference()
                assert ref.kept == 5003 == ref.kept_lo == ref.kept_hi, (c.name, ref)


def test_every_noise_case_is_compared_and_means_what_it_says():
    cases = sp.cases_of("noise")
    assert len(cases) == 2 * (1 + 2 * 7 + 2 * 6)
    for case in cases:
        ref = case.reference()
        assert ref.stable and ref.gap > sp.EPS and ref.token == case.token, (case.name, ref)
        values, ids = case.layout()
        g = sp.step_gumbel(case.step)
        if case.name.startswith("A"):
            assert abs(ref.gap - 0.306) < 1e-3 and values[ids == case.token][0] == -19.5 > -21.0
        if case.name.startswith("B"):
            # 0.01 above the runner-up: over EPS, under the 0.06 the bound has in hand where 1 - u is smallest
            assert abs(ref.gap - 0.01) < 1e-5 and sp.EPS < ref.gap < 17.39 - 17.3287
            if "a-14" in case.name:
                assert values[ids == case.token][0] == -14.0 and values.max() == 0.0
            else:
                rival = ids[np.argmax(values)] if "fill" not in case.name else int(np.argmax(values))
                assert abs(g[rival] - 0.3665) < 0.02
        if case.name.startswith("C"):
            assert abs(ref.gap - 2e-3) < 1e-5


def test_five_and_five_plus_two_to_the_32_differ_on_the_host():
    pairs = 0
    for a in sp.cases_of("seeds"):
        if a.params.seed == 5:
            b = sp.CASES[a.name.replace("seed 0x5 ", f"seed {5 + (1 << 32):#x} ")]
            assert np.array_equal(a.row("inf")[0], b.row("inf")[0])
            assert a.reference().token != b.reference().token, a.name
            pairs += 1
    assert pairs == 4


# ---- teeth --------------------------------------------------------------------------------------------------------------------
def _cases_with(fault):
    cases = [c for c in sp.CASES.values() if c.fault == fault]
    assert cases
    return cases


def test_tooth_truncating_the_level_0_set_at_the_capacity():
    cases = _cases_with("truncate")
    assert {c.block for c in cases} == {"capacity", "past"}
    for case in cases:
        row, _ = case.row("inf")
        right = sp.selected(row, case.params)[:2]
        wrong = sp.selected(row, case.params, truncate=sp.CAP)[:2]
        assert right[1] == case.reference().kept, case.name
        assert wrong != right, case.name
        if case.params.top_k > sp.CAP:        # more ids than the capacity cannot come out of it
            assert wrong[1] != right[1], case.name
    # every case past the capacity is one of them
    assert all(c.fault == "truncate" for c in sp.cases_of("past"))
    assert all((c.fault == "truncate") == (c.n_ge > sp.CAP) for c in sp.cases_of("capacity"))


def test_tooth_dropping_the_lowest_radix_level():
    cases = [c for c in sp.cases_of("levels") if "low_level_only" in c.name]
    assert len(cases) == 8
    for case in cases:
        row, _ = case.row("inf")
        right = sp.selected(row, case.params)[1]
        wrong = sp.selected(row, case.params, drop_low=10)[1]
        assert right == case.reference().kept, case.name
        if case.digits[2] == 0:               # the k-th key is the lowest of the row: everything is kept either way
            assert case.fault is None and right == wrong == 8131, case.name
        else:
            assert case.fault == "drop_low" and wrong == 8131 > right, case.name
    for case in sp.cases_of("levels"):        # the middle level likewise
        if "mid_level_only" in case.name and case.digits[1]:
            row, _ = case.row("inf")
            assert sp.selected(row, case.params, drop_low=21)[1] == 8131 > sp.selected(row, case.params)[1], case.name


def test_tooth_keys_of_negative_floats_without_the_inversion():
    mirrored = [c for c in sp.CASES.values() if c.block in ("capacity", "past", "levels") and " -" in c.name]
    cases = _cases_with("inversion") + mirrored
    assert len(mirrored) >= 30
    for case in cases:
        row, _ = case.row("inf")
        kth, kept, keys = sp.selected(row, case.params)
        if kept == keys.size:                 # a cut that drops nothing cannot tell the orders apart
            assert case.digits and list(case.digits.values()) == [0], case.name
            continue
        wth, _, wkeys = sp.selected(row, case.params, key_of=sp.fkey_without_inversion)
        assert not np.array_equal(keys >= kth, wkeys >= wth), case.name


def test_tooth_half_the_seed_and_the_counters_high_bits():
    for case in _cases_with("seed_hi"):
        row, _ = case.row("inf")
        p = case.params
        low = SamplingParams(p.temperature, p.top_k, p.top_p, p.min_p, p.seed & 0xFFFFFFFF)
        assert sample_host(row, low, case.step, case.stream).token != case.reference().token, case.name
    for case in _cases_with("counter"):
        row, _ = case.row("inf")
        want = case.reference().token
        assert sample_host(row, case.params, case.step & 0xFFFF, case.stream & 0xFFFF).token != want, case.name
        if case.step > 0xFFFF:
            assert sample_host(row, case.params, case.step & 0xFFFF, case.stream).token != want, case.name
        if case.stream > 0xFFFF:
            assert sample_host(row, case.params, case.step, case.stream & 0xFFFF).token != want, case.name


def test_tooth_a_planted_ids_noise_0_02_lower():
    cases = _cases_with("noise_low")
    assert len(cases) == 2 * 2 * 7
    for case in cases:
        values, ids = case.layout()
        keys = values.astype(np.float64) - values.max() + sp.step_gumbel(case.step)[ids]
        assert int(ids[np.argmax(keys)]) == case.token, case.name
        keys[ids == case.token] -= 0.02
        assert int(ids[np.argmax(keys)]) != case.token, case.name
