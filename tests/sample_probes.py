"""Inputs that steer crag_enc_sample (csrc/crag_sample.hip) onto the paths random rows do not reach, and a small model of
which path a row takes.  tests/test_sample_probes_host.py proves the conditions without a GPU; tests/test_sample_probes_gpu.py
runs the same cases through ops.sample.  The reference is sampling.sample_host (fp64) throughout.

The kernel's layout is restated here (LEVEL_BITS, CAP), as decode_probes restates SPLIT and TILE: a logit becomes the
order-preserving key of crag_enc_common.h; the radix selection walks it in digits of 11, 11 and 10 bits; behind the first
level of either selection the ids at or above the chosen bin (n_ge) are copied into LDS when n_ge <= CAP, and stay on the
row otherwise.

A case is a set of candidate logits at chosen ids of a vocabulary; every other id is `off`.  It has two forms with the
same candidates, hence one reference: "inf" (the off ids hold -inf and NaN, no allowed_bits) and "bits" (the off ids
hold logits that would change every answer -- the largest float, NaN, the row's own top values -- and allowed_bits bans
them)."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from cadence_rag_amd.sampling import HostDraw, SamplingParams, min_p_cut, philox4x32_10, sample_host

LEVEL_BITS = (11, 11, 10)       # select(): shift 21, 10, 0
LEVEL_SHIFT = (21, 10, 0)
CAP = 4096                      # SAMPLE_CAP
THREADS = 1024                  # SAMPLE_THREADS: a thread reads the ids congruent to it, in ascending order
VOCAB = 151_936
DELTA, EPS = 1e-4, 1e-3         # test_sample_gpu.py's figures
FLT_MAX = float(np.finfo(np.float32).max)
F32 = np.float32


# ---- the key ----------------------------------------------------------------------------------------------------------
def fkey_host(x) -> np.ndarray:
    """uint32 keys in the order of the floats, -0 folded into +0."""
    b = np.atleast_1d(np.asarray(x, dtype=F32)).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def fkey_without_inversion(x) -> np.ndarray:
    """The fault: a negative float keeps its magnitude bits, so it sorts as its absolute value."""
    b = np.atleast_1d(np.asarray(x, dtype=F32)).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    return (b | np.uint32(0x80000000)).astype(np.uint32)


def from_bits(bits) -> np.ndarray:
    return np.asarray(bits, dtype=np.uint32).view(F32)


def digit(key: int, level: int) -> int:
    return (int(key) >> LEVEL_SHIFT[level]) & ((1 << LEVEL_BITS[level]) - 1)


# ---- the path model ---------------------------------------------------------------------------------------------------
class Sel(NamedTuple):
    key: int                        # the chosen key: the k-th largest, or top-p's threshold
    bin0: int                       # its level-0 digit
    n_ge: int                       # the ids of the selection at or above that bin
    compacts: bool                  # the kernel copies them into LDS behind this level 0
    from_lds: bool                  # the selection already runs over LDS (an earlier selection compacted)
    digit1: int
    digit2: int
    occupied: Tuple[int, int, int]  # per level, the distinct digits among the keys that share the chosen key's prefix


class Path(NamedTuple):
    count: Optional[Sel]            # None: top_k is off, or cuts nothing
    weight: Optional[Sel]           # None: top_p == 1


def _sel(keys: np.ndarray, chosen: int, from_lds: bool) -> Sel:
    keys = keys.astype(np.uint64)
    bin0 = chosen >> 21
    n_ge = int(((keys >> np.uint64(21)) >= bin0).sum())
    occupied = []
    for level in range(3):
        above = LEVEL_SHIFT[level] + LEVEL_BITS[level]
        share = keys if level == 0 else keys[(keys >> np.uint64(above)) == (chosen >> above)]
        occupied.append(int(np.unique((share >> np.uint64(LEVEL_SHIFT[level])) & np.uint64((1 << LEVEL_BITS[level]) - 1)).size))
    return Sel(int(chosen), int(bin0), n_ge, (not from_lds) and n_ge <= CAP, from_lds, digit(chosen, 1), digit(chosen, 2),
               tuple(occupied))


def selected(row, params: SamplingParams, allowed=None, key_of: Callable = fkey_host, drop_low: int = 0,
             truncate: Optional[int] = None) -> Tuple[Optional[int], Optional[int], np.ndarray]:
    """The count selection as an integer model: (the k-th key or None, the kept count or None, the keys of the
    selection).  The faults of the host file's teeth: key_of (another key), drop_low (the lowest bits of the key are not
    looked at), truncate (only that many ids of the level-0 set survive, the lowest ids first as a thread order would)."""
    l32 = np.asarray(row, dtype=F32)
    cand = ~np.isnan(l32) & (l32 != -np.inf)
    if allowed is not None:
        cand &= np.asarray(allowed, dtype=bool)
    if not cand.any():
        return None, None, np.zeros(0, np.uint32)
    m = l32[cand].max()
    with np.errstate(over="ignore", invalid="ignore"):
        cand &= (l32 - m) >= min_p_cut(params.temperature, params.min_p)
    keys = key_of(l32[cand])
    k = int(params.top_k)
    if not (0 < k < l32.size and k < keys.size):
        return None, int(keys.size), keys
    seen = (keys >> np.uint32(drop_low)) << np.uint32(drop_low)
    kth = int(np.sort(seen)[-k])
    if truncate is not None:
        ge = np.nonzero((seen >> np.uint32(21)) >= (kth >> 21))[0][:truncate]
        seen = seen[ge]
        kth = int(np.sort(seen)[-min(k, seen.size)])
    return kth, int((seen >= kth).sum()), keys


def path_of(row, params: SamplingParams, allowed=None) -> Path:
    """Which way the kernel takes this row: see Sel.  The weight selection is computed in fp64 (sample_host's own
    arithmetic); cases rely on it only where sample_host is stable."""
    kth, _, keys = selected(row, params, allowed)
    count = None if kth is None else _sel(keys, kth, False)
    weight = None
    top_p = float(F32(params.top_p))
    if top_p < 1.0 and keys.size:
        temperature = float(F32(params.temperature))
        floor = 0 if kth is None else kth
        inside = keys[keys >= floor]
        from_lds = bool(count and count.compacts)
        if from_lds:                # the pairs in LDS are the level-0 set; the floor still applies
            inside = inside[(inside >> np.uint32(21)) >= count.bin0]
        levels, inverse = np.unique(inside, return_inverse=True)
        values = np.where(levels & np.uint32(0x80000000), levels & np.uint32(0x7fffffff), ~levels).view(F32).astype(np.float64)
        w = np.exp((values - values.max()) / temperature)
        # the maximum of the row is kept by every cut, so values.max() is m
        reach = np.cumsum(np.bincount(inverse, weights=w[inverse], minlength=levels.size)[::-1])
        at = int(np.searchsorted(reach, top_p * reach[-1], side="left"))
        weight = _sel(inside, int(levels[::-1][min(at, levels.size - 1)]), from_lds)
    return Path(count, weight)


# ---- candidate values ---------------------------------------------------------------------------------------------------
def _base_bits(base: float) -> int:
    bits = int(F32(base).view(np.uint32))
    assert bits & 0x1FFFFF == 0, "the base leaves the low 21 bits free"
    return bits


def one_bin(n: int, base: float = 1.0) -> np.ndarray:
    """base + j ulp for n distinct j spread over the low 21 bits: one level-0 digit for the whole row, every lower digit
    in use.  A negative base mirrors the row (the j-th value is the j-th below base)."""
    j = (np.arange(n, dtype=np.uint64) * np.uint64(514_229) + np.uint64(77)) % np.uint64(1 << 21)   # odd stride: distinct
    return from_bits((np.uint64(_base_bits(base)) + j).astype(np.uint32))


def low_level_only(n: int, base: float = 1.0) -> np.ndarray:
    """Values that differ in the low 10 bits alone: n / 1024 ids on each of the 1024 digits of level 2."""
    return from_bits((np.uint64(_base_bits(base)) + np.arange(n, dtype=np.uint64) % np.uint64(1024)).astype(np.uint32))


def mid_level_only(n: int, base: float = 1.0) -> np.ndarray:
    """Values that differ in bits 10..20 alone (the low 10 bits are 0x155 everywhere): n / 2048 ids on each digit of level 1."""
    d = np.arange(n, dtype=np.uint64) % np.uint64(2048)
    return from_bits((np.uint64(_base_bits(base)) + (d << np.uint64(10)) + np.uint64(0x155)).astype(np.uint32))


DENORM_MIN = float(from_bits([1])[0])
NEG_DENORM = float(from_bits([0x80000000 | 0x2ABCD])[0])     # a negative denormal in the middle of the row's


def around_zero(n: int) -> np.ndarray:
    """From the top: larger positives, small normals, denormals (the smallest 40 times), 2 * (n // 3) zeros of both signs,
    the mirror image below them.  The zeros alone are more than CAP ids for n >= 6147."""
    rng = np.random.default_rng(n)
    zeros = n // 3
    side = (n - 2 * zeros) // 2

    def half(count):
        small = count // 4
        den = rng.integers(2, 1 << 23, count // 4, dtype=np.uint32)
        den[:40] = 1
        den[40:44] = 0x2ABCD
        normal = from_bits(rng.integers(0x00800000, 0x01800000, small, dtype=np.uint32))
        large = np.abs(rng.standard_normal(count - small - den.size) * 5 + 0.01).astype(F32)
        return np.concatenate([large, normal, from_bits(den)])

    out = np.concatenate([half(side), np.zeros(zeros, F32), -np.zeros(zeros, F32), -half(n - 2 * zeros - side)])
    assert out.size == n
    return out.astype(F32)


def tied_block(n: int, n_tied: int, value: float, n_above: int = 1, spread: float = 4.0) -> np.ndarray:
    """n_tied ids at value, n_above distinct ones within 1 above it, the rest between 1 and 1 + spread below it."""
    rng = np.random.default_rng(n * 31 + n_tied)
    above = (value + np.linspace(0.25, 1.0, n_above)).astype(F32)
    below = (value - 1.0 - rng.random(n - n_tied - n_above) * spread).astype(F32)
    return np.concatenate([above, np.full(n_tied, value, F32), below])


def normal_row(n: int, seed: int, sd: float = 3.0) -> np.ndarray:
    return (np.random.default_rng(seed).standard_normal(n) * sd).astype(F32)


def top_k_landing_on(values: np.ndarray, value: float) -> int:
    """A top_k whose k-th largest candidate is `value`: one more than the candidates above it."""
    assert (values == F32(value)).any()
    return int((values > F32(value)).sum()) + 1


# ---- the noise --------------------------------------------------------------------------------------------------------
# (step, id) whose 24-bit draw k = x0 >> 8 is extreme, for seed 17, stream 0 and ids below VOCAB; found once with
# philox4x32_10, verified by the host test.
NOISE_SEED = 17
NOISE: Dict[str, List[Tuple[int, int]]] = {
    "top": [(17, 20276), (131, 2339), (132, 92118)],                         # k == 0xFFFFFF: Gumbel 17.3287
    "near_top": [(1, 104123), (4, 110963), (12, 450), (17, 78060)],          # k in 0xFFFFF0..0xFFFFFE
    "zero": [(126, 145254), (216, 27580)],                                   # k == 0: Gumbel -2.852
    "below_half": [(108, 117559), (231, 73508)],                             # k == 2^23 - 1: the last of logf's branch
    "half": [(232, 37250), (233, 129045)],                                   # k == 2^23: the first of log1pf's
}
NOISE_K = {"top": (0xFFFFFF, 0xFFFFFF), "near_top": (0xFFFFF0, 0xFFFFFE), "zero": (0, 0),
           "below_half": ((1 << 23) - 1, (1 << 23) - 1), "half": (1 << 23, 1 << 23)}
LOWEST_U = (17, 96592)          # the id with the smallest u of step 17: u = 6.7e-6, Gumbel -2.4776


def draw_k(seed: int, step: int, stream: int, ids) -> np.ndarray:
    ids = np.asarray(ids, dtype=np.uint64)
    return philox4x32_10((ids, int(step), int(stream), 0), (int(seed) & 0xFFFFFFFF, int(seed) >> 32))[:, 0] >> np.uint32(8)


def gumbel_of_k(k) -> np.ndarray:
    return -np.log(-np.log((np.asarray(k, dtype=np.float64) + 0.5) * 2.0 ** -24))


@functools.lru_cache(maxsize=None)
def step_gumbel(step: int) -> np.ndarray:
    """The Gumbel value of every id of the vocabulary in a step of the noise cases (read-only)."""
    g = gumbel_of_k(draw_k(NOISE_SEED, step, 0, np.arange(VOCAB)))
    g.setflags(write=False)
    return g


# ---- cases --------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    block: str
    v: int
    params: SamplingParams
    build: Callable[[], Tuple[np.ndarray, Optional[np.ndarray]]]   # candidate values, and their ids (None: spread by seed)
    step: int = 3
    stream: int = 1
    count: Optional[str] = None     # expected: None (no count cut), "lds" (compacts behind level 0), "row" (never)
    weight: Optional[str] = None    # expected: None, "lds" (compacts behind top-p's level 0), "row", "held" (already in LDS)
    occupied: Optional[Tuple[int, int, int]] = None      # expected Sel.occupied of the count selection
    digits: Dict[int, int] = field(default_factory=dict)  # expected digit of the k-th key per level
    n_ge: Optional[int] = None      # expected n_ge of the count selection
    sure: bool = False              # compared by the rule of the draw test (stable, gap > EPS, kept in the band)
    token: Optional[int] = None     # the token the construction intends
    fault: Optional[str] = None     # which tooth of the host file bites here
    top_last: bool = False          # the two largest values sit on the two highest candidate ids
    row_key: Optional[str] = None   # seeds block: the entry of ROW_SEEDS

    def layout(self) -> Tuple[np.ndarray, np.ndarray]:
        values, ids = self.build()
        values = np.asarray(values, dtype=F32)
        if ids is None:
            ids = np.sort(np.random.default_rng(self.v + values.size).permutation(self.v)[:values.size])
            values = values[np.random.default_rng(values.size).permutation(values.size)]
            if self.top_last:
                for slot, src in zip((-1, -2), np.argsort(values, kind="stable")[::-1][:2]):
                    values[[slot, src]] = values[[src, slot]]
        assert values.size == len(ids) <= self.v
        return values, np.asarray(ids, dtype=np.int64)

    def row(self, form: str) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """(logits [v], allowed [v] or None)."""
        values, ids = self.layout()
        on = np.zeros(self.v, bool)
        on[ids] = True
        off = np.nonzero(~on)[0]
        row = np.empty(self.v, F32)
        row[ids] = values
        if form == "inf":
            row[off] = np.where(off % 2 == 0, -np.inf, np.nan).astype(F32)
            return row, None
        assert form == "bits"
        finite = values[np.isfinite(values)]
        poison = np.array([FLT_MAX, np.nan, finite.max() if finite.size else 0.0, 0.0, -np.inf,
                           np.median(finite) if finite.size else 1.0], F32)
        row[off] = poison[off % poison.size]
        return row, on

    def reference(self) -> HostDraw:
        return _reference(self.name)


CASES: Dict[str, Case] = {}


@functools.lru_cache(maxsize=None)
def _reference(name: str) -> HostDraw:
    case = CASES[name]
    row, _ = case.row("inf")
    return sample_host(row, case.params, case.step, case.stream, delta=DELTA)


def _add(case: Case) -> None:
    assert case.name not in CASES, case.name
    CASES[case.name] = case


def P(temperature=0.7, **kw) -> SamplingParams:
    kw.setdefault("seed", 5)
    return SamplingParams(temperature, **kw)


def _selection_cases() -> None:
    # -- the capacity edge: 4096 candidates fill LDS exactly, 4097 stay on the row
    for base in (1.0, -1.0):
        for n, v in ((4096, 4096), (4097, 4097), (4096, 4160), (4097, 4161)):
            for k in (1, 2, 4095) + ((4096,) if n == 4097 else ()):
                for mp in (0.0, 0.05):
                    _add(Case(f"edge {base:+g} n{n} v{v} k{k} mp{mp}", "capacity", v, P(top_k=k, min_p=mp),
                              functools.partial(lambda n, base: (one_bin(n, base), None), n, base),
                              count="lds" if n == 4096 else "row", n_ge=n, occupied=(1, None, None),
                              top_last=True, fault="truncate" if n > CAP else None))
    # -- past capacity
    n, v = 8131, 8192
    for base in (1.0, -1.0):
        for k in (1, 2, 4097, 5000, n - 1):
            _add(Case(f"past one_bin {base:+g} k{k}", "past", v, P(top_k=k),
                      functools.partial(lambda base: (one_bin(8131, base), None), base), count="row", n_ge=n,
                      occupied=(1, None, None), top_last=True, fault="truncate"))
    for value in (2.0, -2.0):
        for k in (2, 4999):
            _add(Case(f"past tied {value:+g} k{k}", "past", v, P(top_k=k),
                      functools.partial(lambda value: (tied_block(8131, 5000, value), None), value), count="row", n_ge=5001,
                      fault="truncate"))
    # -- level edges: the k-th key's deciding digit is the first, the second, the last but one and the last of its level
    for base in (1.0, -1.0):
        for builder, level, width in ((low_level_only, 2, 1024), (mid_level_only, 1, 2048)):
            values = builder(n, base)
            keys = fkey_host(values)
            for d in (0, 1, width - 2, width - 1):
                hit = values[np.nonzero([digit(q, level) == d for q in keys[:2 * width]])[0][0]]
                occupied = (1, 1, 1024) if level == 2 else (1, 2048, 1)
                _add(Case(f"{builder.__name__} {base:+g} digit{d}", "levels", v, P(top_k=top_k_landing_on(values, hit) + 1),
                          functools.partial(lambda builder, base: (builder(8131, base), None), builder, base), count="row",
                          n_ge=n, occupied=occupied, digits={level: d},
                          fault=("drop_low" if d else None) if level == 2 else None))
    values = around_zero(n)
    for name, value in (("negative denormal", NEG_DENORM), ("zero", 0.0), ("smallest denormal", DENORM_MIN),
                        ("smallest negative denormal", -DENORM_MIN)):
        for mp in (0.0, 1e-9):        # T ln 1e-9 = -20.7 under a maximum near 15: only large negatives go
            _add(Case(f"around_zero {name} mp{mp}", "zero", v, P(1.0, top_k=top_k_landing_on(values, value) + 1, min_p=mp),
                      lambda: (around_zero(8131), None), count="row", fault="inversion"))
    # -- the real vocabulary
    # (min_p 1e-5 at T 0.7 keeps the ids within 8.06 of the maximum, a few thousand: with top_k 4096 both cuts act)
    for k in (4096, 4097, 20_000, VOCAB - 1):
        n_k = VOCAB if k == VOCAB - 1 else VOCAB - 997         # top_k == v - 1 cuts one id of a full row
        for mp in (0.0, 1e-5):
            _add(Case(f"vocab k{k} mp{mp}", "vocab", VOCAB, P(top_k=k, min_p=mp),
                      functools.partial(lambda k, n_k: (normal_row(n_k, k), None), k, n_k),
                      count="row" if mp == 0.0 or k == 4096 else None))
    for k in (4097, 50_000):
        _add(Case(f"vocab holes k{k}", "vocab", VOCAB - 5, P(top_k=k),      # 151 931 ids: a partial last mask word
                  functools.partial(lambda k: (normal_row(int(0.7 * VOCAB), k + 1), None), k), count="row"))
    # -- temperature at its limits
    for t in (0.01, 100.0):
        for v_t, n_t in ((4097, 4097), (VOCAB, VOCAB - 997)):
            build = functools.partial(lambda n_t: (normal_row(n_t, n_t + 1), None), n_t)
            for k, mp in ((50, 0.0), (0, 0.05), (n_t - 1, 0.0), (4097 if n_t > 4097 else 7, 0.05)):
                _add(Case(f"T{t:g} v{v_t} k{k} mp{mp}", "temperature", v_t, P(t, top_k=k, min_p=mp), build))
            _add(Case(f"T{t:g} v{v_t} top_p 0.9", "temperature", v_t, P(t, top_p=0.9), build, sure=True))

            def extremes(n_t=n_t):
                x = normal_row(n_t, n_t + 2)
                x[n_t // 3], x[2 * n_t // 3] = FLT_MAX, -FLT_MAX      # l - m is -inf in fp32 for the lower one
                return x, None
            for k, mp in ((0, 0.0), (0, 0.05), (n_t - 1, 0.0)):
                _add(Case(f"T{t:g} v{v_t} extremes k{k} mp{mp}", "temperature", v_t, P(t, top_k=k, min_p=mp), extremes))


def _sure_cases() -> None:
    for k in (4097, 20_000):
        for tp in (0.5, 0.9, 0.99):
            for t in (0.7, 1.5):
                _add(Case(f"sure vocab k{k} p{tp} T{t}", "sure", VOCAB, P(t, top_k=k, top_p=tp, seed=17),
                          functools.partial(lambda s: (normal_row(VOCAB - 997, s), None), int(k + 100 * tp + 10 * t)),
                          count="row", sure=True))
    for base in (16.0, -16.0):
        for tp in (0.5, 0.9):
            _add(Case(f"sure one_bin {base:+g} p{tp}", "sure", 8192, P(1.0, top_p=tp, seed=17),
                      functools.partial(lambda base: (one_bin(8131, base), None), base), weight="row", sure=True))
            _add(Case(f"sure one_bin {base:+g} k5000 p{tp}", "sure", 8192, P(1.0, top_k=5000, top_p=tp, seed=17),
                      functools.partial(lambda base: (one_bin(8131, base), None), base), count="row", weight="row", sure=True))
    for value in (2.0, -2.0):
        for k, tp in ((0, 0.5), (0, 0.9), (6000, 0.5)):
            _add(Case(f"sure tied {value:+g} k{k} p{tp}", "sure", 8192, P(1.0, top_k=k, top_p=tp, seed=17),
                      functools.partial(lambda value: (tied_block(8131, 5000, value, n_above=3), None), value),
                      count="row" if k else None, weight="row", sure=True))


def _with_fill(values: List[float], ids: List[int], seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """The named candidates, and N(max - 30, 2^2) on every other id: candidates that cannot win."""
    row = (max(values) - 30.0 + 2.0 * np.random.default_rng(seed).standard_normal(VOCAB)).astype(F32)
    row[ids] = values
    return row, np.arange(VOCAB)


def _noise_case(name: str, step: int, ids: List[int], values: List[float], token: int, fault: Optional[str] = None) -> None:
    params = SamplingParams(1.0, seed=NOISE_SEED)
    _add(Case(name, "noise", VOCAB, params, lambda: (np.asarray(values, F32), np.asarray(ids)), step=step, stream=0,
              token=token, fault=fault))
    _add(Case(name + " fill", "noise", VOCAB, params, lambda: _with_fill(values, ids, step), step=step, stream=0, token=token,
              fault=fault))


def _first(step: int, ok: np.ndarray, start: int = 0, same_thread_below: Optional[int] = None) -> int:
    """The first id from `start` on that satisfies ok; with same_thread_below, a lower id of the same thread if one does."""
    if same_thread_below is not None:
        mine = np.arange(same_thread_below % THREADS, same_thread_below, THREADS)
        if ok[mine].any():
            return int(mine[ok[mine]][0])
    idx = np.nonzero(np.roll(ok, -start))[0]
    return int((idx[0] + start) % ok.size)


def _noise_cases() -> None:
    # A: the maximum on the lowest u of the step, a challenger 19.5 below it on the highest: above SAMPLE_SKIP, and it wins
    step, top = NOISE["top"][0]
    assert LOWEST_U[0] == step
    _noise_case("A skip and first bound", step, [LOWEST_U[1], top], [0.0, -19.5], top)
    # B: the planted id's key leads the runner-up's by 0.01, inside the 0.06 gumbel_bound has in hand
    for kind in ("top", "near_top"):
        for step, planted in NOISE[kind]:
            g = step_gumbel(step)
            taken = np.zeros(VOCAB, bool)
            taken[planted] = True
            # a = -14 under a maximum at 0: the runner-up's logit must stay below 0, so its own noise is high (u > 0.97)
            key = -14.0 + g[planted]
            rival = _first(step, (g > key - 0.01 + 0.05) & (g < key - 0.01 + 3.0) & ~taken, same_thread_below=planted)
            taken[rival] = True
            anchor = _first(step, (g < key - 1.5) & ~taken, start=(planted + 512) % VOCAB)
            _noise_case(f"B a-14 {kind} step{step}", step, [anchor, planted, rival], [0.0, -14.0, key - 0.01 - g[rival]],
                        planted, fault="noise_low")
            # the runner-up is the maximum itself, on a u near one half; the planted id then sits near a = -16.95
            taken[:] = False
            taken[planted] = True
            rival = _first(step, (np.abs(g - 0.3665) < 0.02) & ~taken, same_thread_below=planted)
            _noise_case(f"B half {kind} step{step}", step, [rival, planted], [0.0, g[rival] + 0.01 - g[planted]], planted,
                        fault="noise_low")
    # C: the two formulas of gumbel() meet, and the lowest value there is
    for kind in ("below_half", "half", "zero"):
        for step, special in NOISE[kind]:
            g = step_gumbel(step)
            taken = np.zeros(VOCAB, bool)
            taken[special] = True
            other = _first(step, (np.abs(g) < 2.0) & ~taken, start=(special + 1000) % VOCAB)
            for order, lead in (("wins", -2e-3), ("loses", 2e-3)):
                _noise_case(f"C {kind} step{step} {order}", step, [special, other], [0.0, g[special] - g[other] + lead],
                            special if lead < 0 else other)


# the seed of each row of the seed / counter block where it is not 0: the first on which the host is sure of every case
# that shares the row and every tooth of the host file bites (the host file asserts both)
ROW_SEEDS: Dict[str, int] = {
    "counter step0x80000000 stream0x80000000 v1025 k50": 2,
    "counter step0x80000000 stream0xffffffff v1025 k50": 4,
    "counter step0xffffffff stream0xffffffff v1025 k50": 2,
    "counter step0x7 stream0xffffffff v1025 k50": 1,
    "counter step0xffffffff stream0x80000000 v151936 plain": 1,
    "seed 0x100000000 v151936 k50": 1,
    "seed 0x123456789abcdef v151936 k50": 1,
    "counter step0x80000000 stream0xffffffff v151936 k50": 1,
    "counter step0xffffffff stream0x80000000 v151936 k50": 1,
}
SEEDS = (1 << 32, (1 << 64) - 1, 0x0123456789ABCDEF, 5, 5 + (1 << 32))
COUNTERS = [(step, stream) for step in (1 << 31, (1 << 32) - 1, 7) for stream in (1 << 31, (1 << 32) - 1, 7)][:-1]


def _seed_cases() -> None:
    for v in (1025, VOCAB):
        for tag, kw in (("plain", dict(temperature=1.0)), ("k50", dict(temperature=0.7, top_k=50))):
            for seed in SEEDS:
                name = f"seed {seed:#x} v{v} {tag}"
                key = f"seed {seed & 0xFFFFFFFF:#x} v{v} {tag}" if seed == 5 + (1 << 32) else name   # 5 and 5 + 2^32: one row
                _add(Case(name, "seeds", v, SamplingParams(seed=seed, **kw),
                          functools.partial(lambda v, key: (normal_row(v, ROW_SEEDS.get(key, 0)), None), v, key),
                          step=3, stream=1, sure=True, fault="seed_hi" if seed >> 32 else None, row_key=key))
            for step, stream in COUNTERS:
                name = f"counter step{step:#x} stream{stream:#x} v{v} {tag}"
                _add(Case(name, "seeds", v, SamplingParams(seed=17, **kw),
                          functools.partial(lambda v, name: (normal_row(v, ROW_SEEDS.get(name, 0)), None), v, name),
                          step=step, stream=stream, sure=True, fault="counter", row_key=name))


_selection_cases()
_sure_cases()
_noise_cases()
_seed_cases()
BLOCKS = ("capacity", "past", "levels", "zero", "vocab", "temperature", "sure", "noise", "seeds")
EXACT_BLOCKS = ("capacity", "past", "levels", "zero", "vocab", "temperature")
assert {c.block for c in CASES.values()} == set(BLOCKS)


def cases_of(block: str) -> List[Case]:
    return [c for c in CASES.values() if c.block == block]


def calls_of(block: str, rows: int) -> List[List[Case]]:
    """The cases of a block as calls of `rows` rows: one vocabulary, seed and step a call; a short call is filled up with
    the cases before it, so a call of 8 is always 8 mixed rows."""
    groups: Dict[tuple, List[Case]] = {}
    for c in cases_of(block):
        groups.setdefault((c.v, int(c.params.seed), c.step), []).append(c)
    calls = []
    for members in groups.values():
        for lo in range(0, len(members), rows):
            call = members[lo:lo + rows]
            calls.append(call + [members[(lo - 1 - i) % len(members)] for i in range(rows - len(call))])
    return calls
