"""The guards of the attention probes (tests/attention_probes.py), for every case tests/test_attention_probes_gpu.py runs,
on the CPU: a selection probe's off-target softmax mass is <= 2^-20 (2^-24 for the fused kernels of <= 32 tokens), and a
lure probe's forbidden key, were it let in, would move its row by more than ten times the comparison's bar."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import attention_probes as ap


def _select_mass(lens, parent, hq, hkv, maps, seed):
    worst, seen = 0.0, set()
    for lay, names, tgt, qkv in ap.launches(lens, parent, hq, hkv, maps, seed, lure=False):
        q, k, v = ap.split(qkv, hq, hkv, lay.t)
        assert torch.isnan(k[lay.t:]).all()                                  # the rows past T stay NaN
        mass = ap.selection_mass(q, k, v, lay.allowed, tgt)
        worst = max(worst, float(mass.max()))
        seen.update(names)
        assert all(a != b for a, b in zip(names, names[1:]))                 # head 0 never shares a map with head 1
    assert seen == set(maps)                                                 # every map runs in some launch
    return worst


def _lure_ok(lens, parent, hq, hkv, maps, seed):
    tails = []
    for lay, names, forb, qkv in ap.launches(lens, parent, hq, hkv, maps, seed, lure=True):
        q, k, v = ap.split(qkv, hq, hkv, lay.t)
        ref = ap.reference(q, k, v, lay.allowed)
        assert torch.isfinite(ref).all()
        ok = ap.lure_guard(q, k, v, lay.allowed, forb, ref)
        assert ok.all(), (names, torch.nonzero(~ok)[:8].tolist())
        tails.append(bool(torch.isnan(k[lay.t:]).all()))
    assert tails == [True, False] * (len(tails) // 2)                         # each launch: NaN rows past T, then keys


@pytest.mark.parametrize("case", ap.ATTENTION_SELECT, ids=lambda c: c.name)
def test_attention_selection_guard(case):
    assert sum(case.lens) <= 1500
    worst = _select_mass(case.lens, None, case.hq, case.hkv, ap.PLAIN_MAPS, case.seed)
    print(f"\n{case.name}: largest off-target mass 2^{np.log2(worst):.1f}")
    assert worst <= ap.SELECTION_MASS


@pytest.mark.parametrize("case", ap.ATTENTION_LURE, ids=lambda c: c.name)
def test_attention_lure_guard(case):
    _lure_ok(case.lens, None, case.hq, case.hkv, ap.PLAIN_LURES, case.seed)


@pytest.mark.parametrize("case", ap.PREFIXED, ids=lambda c: c.name)
def test_prefixed_selection_guard(case):
    worst = _select_mass(case.lens, case.parent, case.hq, case.hkv, ap.PREFIXED_SELECT_MAPS, case.seed)
    print(f"\n{case.name}: largest off-target mass 2^{np.log2(worst):.1f}")
    assert worst <= ap.SELECTION_MASS


@pytest.mark.parametrize("case", ap.PREFIXED, ids=lambda c: c.name)
def test_prefixed_lure_guard(case):
    _lure_ok(case.lens, case.parent, case.hq, case.hkv, ap.PREFIXED_LURES, case.seed + 1)


def test_prefixed_layout_puts_every_named_key_where_the_issue_wants_it():
    """The forbidden keys of a child: the row behind its parent's last row belongs to the other root, a sibling's key, a
    key of the unrelated root; of a root row: a key of one of its children; the child behind the second root's copy sits
    directly behind its parent."""
    case = ap.PREFIXED[1]
    lay = ap.Layout.build(case.lens, case.parent)
    f = ap.lure_targets(lay, ap.PREFIXED_LURES)
    seq = lay.seq_of
    for b in (2, 3, 4):
        rows = seq == b
        assert (f[rows, 0] == lay.cu[1]).all()                               # first row of the unrelated root
        assert set(seq[f[rows, 1]]) <= {2, 3, 4} - {b}                       # a sibling
        assert (seq[f[rows, 2]] == 1).all()
    assert lay.cu[6] == lay.cu[5] + case.plen and case.parent[6] == 5
    assert (seq[f[seq == 6, 1]] == 4).all() and (seq[f[seq == 6, 0]] == 1).all()
    assert set(seq[f[seq == 0, 0]]) == {2} and set(seq[f[seq == 0, 3]]) == {4}
    assert set(seq[f[seq == 5, 0]]) == {6}


@pytest.mark.parametrize("lens", ap.SMALL_LENS, ids=ap.small_id)
def test_small_selection_guard(lens):
    hq, hkv = ap.SMALL_HEADS
    lay, tgt, qkv, gains = ap.small_inputs(lens, lure=False)
    names = ap.head_maps(ap.SMALL_MAPS, hq)[0]
    assert set(names) == set(ap.SMALL_MAPS) and all(len(set(names[g:g + 4])) == 4 for g in range(0, hq, 4))
    q, k, v = ap.small_qkv_ref(lay, qkv, gains)
    worst = float(ap.selection_mass(q, k, v, lay.allowed, tgt).max())
    print(f"\n{lens}: largest off-target mass 2^{np.log2(max(worst, 1e-300)):.1f}")
    assert worst <= ap.SMALL_SELECTION_MASS
    # the gain is exact: a sign vector has RMS 1 and its normalised elements round to +-1 in bf16
    raw = ap.split(qkv[:lay.t], hq, hkv)[0]
    assert torch.equal((raw * torch.rsqrt(raw.pow(2).mean(-1, keepdim=True) + ap.EPS)).to(ap.BF).float(), raw)


@pytest.mark.parametrize("lens", ap.SMALL_LURE_LENS, ids=ap.small_id)
def test_small_lure_guard(lens):
    lay, forb, qkv, gains = ap.small_inputs(lens, lure=True)
    q, k, v = ap.small_qkv_ref(lay, qkv, gains)
    ref = ap.reference(q, k, v, lay.allowed)
    ok = ap.lure_guard(q, k, v, lay.allowed, forb, ref)
    assert ok.all(), torch.nonzero(~ok)[:8].tolist()
    # the forbidden keys the issue names: the previous sequence's last key and the next one's first, inside one block
    names = ap.head_maps(ap.SMALL_LURES, ap.SMALL_HEADS[0])[0]
    assert names[:4] == list(ap.SMALL_LURES)
    last = lay.t - 1
    assert forb[last, 0] == lay.cu[-2] - 1 and forb[0, 1] == lay.cu[1]


def test_one_wrong_mask_comparison_is_what_the_widened_reference_computes():
    """A kernel whose causal test read `key > q0 + c + 1` would let exactly key i + 1 in, for every row but the last of a
    32-key tile (whose next key lies in a tile that is not walked): for the 'next' lure that is the widened mask of the
    guard, so each of those rows would miss the bar by the guard's factor of ten."""
    case = ap.ATTENTION_LURE[0]
    lay, names, forb, qkv = list(ap.launches(case.lens, None, case.hq, case.hkv, ap.PLAIN_LURES, case.seed, lure=True))[1]  # keys past T
    h = names.index("next")
    assert (forb[:, h] == np.arange(lay.t) + 1).all()
    off_by_one = lay.allowed.clone()
    rows = torch.arange(lay.t)
    off_by_one[rows, rows + 1] = True                                        # what such a kernel would compute
    q, k, v = ap.split(qkv, case.hq, case.hkv, lay.t)
    ref, wrong = ap.reference(q, k, v, lay.allowed), ap.reference(q, k, v, off_by_one)
    far = ((wrong[:, h] - ref[:, h]).abs() > 10 * (ap.ATOL + ap.RTOL * ref[:, h].abs())).any(-1)
    assert far[lay.local % 32 != 31].all()
