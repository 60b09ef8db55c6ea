"""Exact probes for the encoder's linear layers (skinny_gemm_kernel, small_gemm_kernel, wide_gemm_kernel + wide_reduce_kernel
+ rmsnorm_partials_kernel): construction, exact references, case lists and layout formulas, all on the CPU (this module
never loads the native library; tests/test_gemm_probes_host.py proves the conditions the comparisons rest on without a
GPU, tests/test_gemm_probes_gpu.py runs the same case lists through the kernels).

Random-normal activations against 0.02 * randn weights put one weight element at ~0.02 of an output of standard deviation
~1, below any tolerance.  Here nothing is approximate:

  integer probe    small-integer operands with 24 non-zeros per row on one side: every product and every partial sum is
                   an integer (or a half, with the RMSNorm prologue) far below 2^24, so fp32 accumulation is exact in ANY
                   order, and |sum| <= 144 is bf16-exact (asserted per case on the host: |ref| <= 256 and
                   bf16(ref) == ref), so the kernel's bf16 output must EQUAL the int64 matmul.
  selection probe  activation row m is e_{k_m}: the output row must be W[:, k_m] bit for bit (every other product is
                   +-0), W dense 0.02 * randn.  The k_m walk the K division of the form: first and last column of every
                   wave's / split's / LDS chunk's range, and every in-step position of one middle k-step.
  prologue probe   x, delta integers with |x + delta| = c (a power of two) in a whole row: mean square exactly c^2,
                   bf16((x + delta) * rsqrt(c^2 + 1e-6)) exactly +-1, norm_w in {+-0.5, +-1, +-2}: the GEMM operand is
                   exactly +-norm_w[k] and res_out exactly x + delta.
  SwiGLU           gate and up sums are exact, so the output is pinned to a set: silu(gate) in fp64, its two bf16
                   neighbours a_lo <= silu <= a_hi, {bf16(a * up)} -- one or two members (a bf16 x bf16 product is exact
                   in fp32).  The GPU file also asks for the bits of crag_enc_swiglu on the exact gate|up matrix.  The
                   probes keep |gate| <= 80 (asserted on the host): the kernels' __expf(-gate) overflows fp32 past 88.

All references are carried in HALF units as int64 (`ref2` = 2 * sum), so the prologue's half-integers fit the same code."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

BF = torch.bfloat16
NNZ = 24                      # non-zeros per row of the sparse operand
W_VALUES = (-3.0, -2.0, -1.0, 1.0, 2.0, 3.0)
X_VALUES = (-2.0, -1.0, 1.0, 2.0)
NORM_W_VALUES = (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0)
REF_LIMIT = 256               # integers up to 256 are bf16 values
GATE_LIMIT = 80               # __expf(-gate) stays finite in fp32 (overflows past 88)
WIDE_PAD_VALUE = 3.0          # the wide kernels READ the padding rows: finite
EPS = 1e-6
NOMINAL_CUS = 256             # the host file's stand-in for the device's CU count (MI355X: 256)
MODES = ("dense_w", "sparse_w")


# ----------------------------------------------------------------------------------------------------------------------
# the forms, as data: how each kernel instance divides K (the host file checks the selection columns against these)
# ----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Form:
    family: str                   # "skinny" | "small"
    name: str
    k: int
    rows: int                     # weight rows per n-tile
    swiglu: bool
    prologue: bool
    multi: bool                   # small_gemm_kernel's MULTI_ (grid-stride over the tiles)
    division: Tuple[Tuple[int, Tuple[Tuple[int, int], ...]], ...]   # m_pad -> ((WAVES, KS), ...): K = WAVES * KS * 32
    ns: Tuple[int, ...]           # (skinny) the n of the cases

    def divisions(self, m_pad: int) -> Tuple[Tuple[int, int], ...]:
        return dict(self.division)[m_pad]


_D10 = ((16, ((8, 10),)), (32, ((8, 10),)))
_D16 = ((16, ((8, 16),)), (32, ((8, 16),)))
SKINNY_FORMS = (
    Form("skinny", "skinny-k2560", 2560, 16, False, False, False, _D10, (32, 96)),            # <MG, 2, 10, 8, 0>
    Form("skinny", "skinny-k2560-swiglu", 2560, 16, True, False, False, _D10, (32, 96)),      # <MG, 2, 10, 8, 1>
    Form("skinny", "skinny-k4096", 4096, 16, False, False, False, _D16, (16, 32, 96)),        # <MG, 1, 16, 8, 0>
    Form("skinny", "skinny-k9728", 9728, 16, False, False, False,                             # <1, 1, 38, 8, 0>, <2, 1, 19, 16, 0>
         ((16, ((8, 38),)), (32, ((16, 19),))), (16, 32, 96)),
)
SMALL_FORMS = (
    Form("small", "small-k2560-pro-r12", 2560, 12, False, True, True, _D10, ()),              # <MG, 10, 8, 10, 12, 0, 1, 1, 1>
    Form("small", "small-k2560-pro-swiglu-r16", 2560, 16, True, True, True, _D10, ()),        # <MG, 10, 8, 10, 16, 1, 1, 1, 1>
    Form("small", "small-k4096-r10", 4096, 10, False, False, False, _D16, ()),                # <MG, 16, 8, 16, 10, 0, 0, 0, 1>
    Form("small", "small-k9728-r10", 9728, 10, False, False, False,                           # <1, 38, 8, 19, ...>, <2, 38, 8, 12, ..., XPASS 2>
         ((16, ((8, 38),)), (32, ((8, 38), (16, 19)))), ()),                                  # (XPASS 2: a wave's 38 k-steps in two passes of 19)
)
SMALL_ROWS = ((16, (1, 15, 16)), (32, (17, 31, 32)))      # m_pad -> m_rows (skinny and small)


def small_ns(form: Form, cus: int) -> Tuple[int, ...]:
    """One tile, three tiles and, for the MULTI_ forms, a tile count above the CU count that the CUs do not divide."""
    ns = [form.rows, 3 * form.rows]
    if form.multi:
        tiles = cus + cus // 3 + 1
        assert tiles > cus and tiles % cus != 0
        ns.append(form.rows * tiles)
    return tuple(ns)


def form_ns(form: Form, cus: int) -> Tuple[int, ...]:
    return form.ns if form.family == "skinny" else small_ns(form, cus)


WIDE_TILES = ((128, 128), (64, 64))                        # (CRAG_WIDE_TILE, columns per LDS chunk)
WIDE_K_SPLITS = ((128, 1), (256, 1), (256, 2), (384, 1), (384, 2), (384, 3), (640, 2), (640, 3), (1280, 4))
WIDE_ROWS = ((32, (1, 31, 32)), (64, (1, 31, 63, 64)), (96, (1, 63, 95, 96)), (128, (1, 95, 127, 128)))
WIDE_NS = (128, 384)
WIDE_4B = (9728, 8, 2560)                                  # (k, splitk, n): 76 chunks of 128 split as 9 or 10
WIDE_THRESHOLD = ((512, 4, 128 * 25), (512, 3, 128 * 33))  # (k, splitk, n): (n / 128) * splitk = 100 and 99
WIDE_ENTRIES = ("reduce-0", "reduce-1", "direct-0", "direct-1", "rows")


def wide_entries(splitk: int) -> Tuple[str, ...]:
    """The direct form is the unsplit one."""
    return tuple(e for e in WIDE_ENTRIES if splitk == 1 or not e.startswith("direct"))


def wide_chunks_per_split(k: int, splitk: int, chunk: int) -> List[int]:
    chunks = k // chunk
    return [chunks * (s + 1) // splitk - chunks * s // splitk for s in range(splitk)]


def wide_default_tile(n: int, splitk: int) -> int:
    return 128 if (n // 128) * splitk >= 100 else 64


# ----------------------------------------------------------------------------------------------------------------------
# K ranges
# ----------------------------------------------------------------------------------------------------------------------
def wave_ranges(divisions: Sequence[Tuple[int, int]]) -> List[Tuple[int, int]]:
    """[lo, hi) columns of every wave's K range, for every (WAVES, KS) given."""
    out = []
    for waves, ks in divisions:
        out += [(32 * ks * w, 32 * ks * (w + 1)) for w in range(waves)]
    return sorted(set(out))


def split_ranges(k: int, splitk: int, chunk: int) -> List[Tuple[int, int]]:
    chunks = k // chunk
    return [(chunk * (chunks * s // splitk), chunk * (chunks * (s + 1) // splitk)) for s in range(splitk)]


def form_ranges(form: Form, m_pad: int) -> List[Tuple[int, int]]:
    """The K ranges of the instance's finest division (XPASS halves a wave's range)."""
    return wave_ranges([max(form.divisions(m_pad))])


def form_parts(form: Form) -> int:
    """Equal parts of K that the sparse operand's rows each hit: the finest wave division of the form."""
    return max(w for _, divs in form.division for w, _ in divs)


def wide_parts(k: int) -> int:
    return k // 64 if k // 64 <= 20 else 16


# ----------------------------------------------------------------------------------------------------------------------
# selection columns
# ----------------------------------------------------------------------------------------------------------------------
def form_select_columns(form: Form) -> List[int]:
    """First and last column of every wave's K range (of every instance of the form) and the 32 positions 8 g + e of the
    middle k-step."""
    cols = set()
    for _, divs in form.division:
        for lo, hi in wave_ranges(divs):
            cols.update((lo, hi - 1))
    mid = 32 * (form.k // 64)
    cols.update(range(mid, mid + 32))
    return sorted(cols)


def wide_select_columns(k: int, splitk: int) -> List[int]:
    """First and last column of every LDS chunk at both chunk widths (a split's range is a run of chunks, so these hold
    every split's edges) and the 16 positions 8 h + e of the middle 16-wide k-step."""
    cols = set()
    for _, chunk in WIDE_TILES:
        for c in range(k // chunk):
            cols.update((chunk * c, chunk * (c + 1) - 1))
        for lo, hi in split_ranges(k, splitk, chunk):
            cols.update((lo, hi - 1))
    mid = 16 * (k // 32)
    cols.update(range(mid, mid + 16))
    return sorted(cols)


def selection_launches(cols: Sequence[int], m_rows: int) -> List[List[int]]:
    """The columns dealt over launches of m_rows rows; the last launch wraps round to the first columns."""
    out = []
    for i in range(0, len(cols), m_rows):
        grp = list(cols[i:i + m_rows])
        grp += [cols[j % len(cols)] for j in range(m_rows - len(grp))]
        out.append(grp)
    return out


def selection_weight(n: int, k: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, k, generator=g) * 0.02).to(BF)


def one_hot(cols: Sequence[int], m_pad: int, k: int, pad: float) -> torch.Tensor:
    x = torch.zeros(m_pad, k, dtype=BF)
    x[torch.arange(len(cols)), torch.tensor(cols)] = 1.0
    x[len(cols):] = pad
    return x


# ----------------------------------------------------------------------------------------------------------------------
# integer and prologue operands
# ----------------------------------------------------------------------------------------------------------------------
def _seed(*key) -> int:
    return zlib.crc32(repr(key).encode())


def _draw(values: Sequence[float], shape, g) -> torch.Tensor:
    v = torch.tensor(values)
    return v[torch.randint(0, len(values), shape, generator=g)]


def _sparse(rows: int, k: int, parts: int, values: Sequence[float], g) -> torch.Tensor:
    """[rows, k] with exactly NNZ non-zeros per row from all of [0, k): one in each of `parts` equal parts of K, the rest
    anywhere else."""
    assert parts <= NNZ and k % parts == 0
    width = k // parts
    first = torch.randint(0, width, (rows, parts), generator=g) + width * torch.arange(parts)
    score = torch.rand(rows, k, generator=g)
    score.scatter_(1, first, -1.0)
    cols = torch.cat([first, score.topk(NNZ - parts, dim=1).indices], dim=1)
    out = torch.zeros(rows, k)
    out.scatter_(1, cols, _draw(values, (rows, NNZ), g))
    return out


@dataclass
class Operands:
    x: torch.Tensor               # [rows, k] bf16: what the kernel is given (prologue: the residual stream)
    w: torch.Tensor               # [n, k] bf16, torch Linear layout (SwiGLU: gate rows, then up rows)
    xop2: torch.Tensor            # [rows, k] int64: TWICE the GEMM's exact B operand
    ref2: torch.Tensor            # [rows, n] int64: twice the exact sums, xop2 @ w^T
    sparse_row0: torch.Tensor     # the non-zero columns of row 0 of the sparse operand
    seed: int
    delta: Optional[torch.Tensor] = None      # prologue: [rows, k] bf16
    norm_w: Optional[torch.Tensor] = None     # prologue: [k] bf16
    res: Optional[torch.Tensor] = None        # prologue: x + delta, [rows, k] bf16


def int_reference(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    return x.long() @ w.long().t()


def _valid(ref2: torch.Tensor, swiglu: bool) -> bool:
    ref = ref2.double() / 2
    if float(ref.abs().max()) > REF_LIMIT or not torch.equal(ref.float().to(BF).double(), ref):
        return False
    return not swiglu or float(ref[:, : ref.shape[1] // 2].abs().max()) <= GATE_LIMIT


@functools.lru_cache(maxsize=6)
def operands(mode: str, k: int, n: int, rows: int, parts: int, swiglu: bool, key: str) -> Operands:
    """The operands of an integer probe (mode "dense_w" / "sparse_w") or of a prologue probe ("prologue": sparse weights),
    `rows` token rows (a case with fewer uses the first ones).  Seeds are tried in order until the exactness conditions
    hold (bf16-exact sums, |gate| <= GATE_LIMIT); the host file asserts them for what comes out."""
    for attempt in range(16):
        seed = _seed(mode, k, n, rows, key, attempt)
        g = torch.Generator().manual_seed(seed)
        delta = norm_w = res = None
        if mode == "dense_w":
            w = _draw(W_VALUES, (n, k), g)
            x = _sparse(rows, k, parts, X_VALUES, g)
            xop2, row0 = (2 * x).long(), torch.nonzero(x[0]).flatten()
        else:
            w = _sparse(n, k, parts, W_VALUES, g)
            row0 = torch.nonzero(w[0]).flatten()
            if mode == "sparse_w":
                x = _draw(X_VALUES, (rows, k), g)
                xop2 = (2 * x).long()
            else:
                c = 2.0 ** torch.randint(0, 4, (rows, 1), generator=g)
                sign = _draw((-1.0, 1.0), (rows, k), g)
                delta = torch.randint(-3, 4, (rows, k), generator=g).float()
                x = sign * c - delta
                norm_w = _draw(NORM_W_VALUES, (k,), g)
                res = sign * c
                xop2 = (2 * sign * norm_w).long()
        ref2 = int_reference(xop2, w)
        if _valid(ref2, swiglu):
            bf = lambda t: None if t is None else t.to(BF)
            return Operands(bf(x), bf(w), xop2, ref2, row0, seed, bf(delta), bf(norm_w), bf(res))
    raise AssertionError(f"no seed gives exact sums for {mode} k={k} n={n}")


def padded(x: torch.Tensor, m_rows: int, m_pad: int, pad: float) -> torch.Tensor:
    out = x[:m_pad].clone()
    out[m_rows:] = pad
    return out


def form_operands(form: Form, n: int, mode: str) -> Operands:
    return operands("prologue" if form.prologue else mode, form.k, n, 32, form_parts(form), form.swiglu, form.name)


def wide_operands(k: int, n: int, mode: str) -> Operands:
    """One operand set serves both epilogues (|gate| <= GATE_LIMIT is asked of its first n / 2 rows of W either way)."""
    return operands(mode, k, n, 128, wide_parts(k), True, "wide")


def form_modes(form: Form) -> Tuple[str, ...]:
    return ("prologue",) if form.prologue else MODES


# ----------------------------------------------------------------------------------------------------------------------
# expected outputs
# ----------------------------------------------------------------------------------------------------------------------
def _bf16_step(a: torch.Tensor, up: bool) -> torch.Tensor:
    """The next bf16 value above (up) or below a bf16 value, through the bits of its fp32 form."""
    f = a.float()
    bits = f.view(torch.int32)
    one = 1 << 16
    away = (bits + one).view(torch.float32)                 # larger magnitude, same sign
    toward = (bits - one).view(torch.float32)               # smaller magnitude (the smallest subnormal -> 0)
    tiny = torch.tensor(one, dtype=torch.int32).view(torch.float32)
    pos, zero = f > 0, f == 0
    nxt = torch.where(pos, away if up else toward, toward if up else away)
    return torch.where(zero, tiny if up else -tiny, nxt).to(BF)


def silu_neighbours(gate: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """a_lo <= silu(gate) <= a_hi, adjacent bf16 values (equal when silu(gate) is one), silu in fp64."""
    g = gate.double()
    s = g / (1.0 + torch.exp(-g))
    c = s.float().to(BF)
    cd = c.double()
    lo = torch.where(cd <= s, c, _bf16_step(c, up=False))
    hi = torch.where(cd >= s, c, _bf16_step(c, up=True))
    assert bool((lo.double() <= s).all()) and bool((s <= hi.double()).all())
    return lo, hi


def swiglu_set(gate: torch.Tensor, up: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The one or two admissible outputs for bf16 gate and up values: bf16(a * up) for a in (a_lo, a_hi)."""
    lo, hi = silu_neighbours(gate)
    u = up.float()
    return (lo.float() * u).to(BF), (hi.float() * u).to(BF)


def pre_activation(ref2: torch.Tensor) -> torch.Tensor:
    """The exact sums as bf16 (what an unfused linear layer would write)."""
    return (ref2.double() / 2).float().to(BF)


def expected(ref2: torch.Tensor, swiglu: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lo, hi): the output must equal one of them; without SwiGLU both are the exact sums."""
    pre = pre_activation(ref2)
    if not swiglu:
        return pre, pre
    inter = pre.shape[1] // 2
    return swiglu_set(pre[:, :inter], pre[:, inter:])


def member(got: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor) -> torch.Tensor:
    g = got.float()
    return (g == lo.float()) | (g == hi.float())


# ----------------------------------------------------------------------------------------------------------------------
# the five weight orders, as index formulas (include/crag_encoder.h), independent of encoder/ops.py
# ----------------------------------------------------------------------------------------------------------------------
def _stream_index(n: int, k: int, rows: int, step: int) -> Tuple[np.ndarray, np.ndarray]:
    """Element p of the stream [n / rows][k / step][step / 8][rows][8] is W[row[p], col[p]]."""
    p = np.arange(n * k, dtype=np.int64)
    e = p % 8
    r = (p // 8) % rows
    g = (p // (8 * rows)) % (step // 8)
    s = (p // (8 * rows * (step // 8))) % (k // step)
    t = p // (rows * step * (k // step))
    return rows * t + r, step * s + 8 * g + e


def _take(weight: torch.Tensor, row: np.ndarray, col: np.ndarray) -> torch.Tensor:
    return weight[torch.from_numpy(row), torch.from_numpy(col)]


def skinny_weight(weight: torch.Tensor) -> torch.Tensor:
    """[n/16][k/32][lane = 16 (kk/8) + row][8] = W[16 tile + row][32 step + 8 (lane >> 4) + e]"""
    return _take(weight, *_stream_index(*weight.shape, 16, 32))


def small_weight(weight: torch.Tensor, rows: int) -> torch.Tensor:
    """[n / rows][k / 32][4][rows][8]"""
    return _take(weight, *_stream_index(*weight.shape, rows, 32))


def wide_weight(weight: torch.Tensor) -> torch.Tensor:
    """[n/32][k/16][lane = 32 (kk/8) + row][8]"""
    return _take(weight, *_stream_index(*weight.shape, 32, 16))


def _gate_up_row(row: np.ndarray, inter: int, feats: int) -> np.ndarray:
    """Streamed row 2 feats t + r is gate row feats t + r (r < feats) or up row feats t + r - feats."""
    t, r = row // (2 * feats), row % (2 * feats)
    return np.where(r < feats, feats * t + r, inter + feats * t + r - feats)


def skinny_gate_up_weight(gate_up: torch.Tensor) -> torch.Tensor:
    """tile t = gate rows 8t..8t+7, then up rows 8t..8t+7, in skinny_weight's order"""
    row, col = _stream_index(*gate_up.shape, 16, 32)
    return _take(gate_up, _gate_up_row(row, gate_up.shape[0] // 2, 8), col)


def wide_gate_up_weight(gate_up: torch.Tensor) -> torch.Tensor:
    """every 32 rows = 16 gate rows then the 16 up rows of the same features, in wide_weight's order"""
    row, col = _stream_index(*gate_up.shape, 32, 16)
    return _take(gate_up, _gate_up_row(row, gate_up.shape[0] // 2, 16), col)


def tile_features(family: str, rows: int, swiglu: bool) -> int:
    """Output features (columns of the torch-layout reference) that share an n-tile: adjacent ones inside such a group are
    adjacent weight rows of one tile."""
    if family == "wide":
        return 16 if swiglu else 32
    return 8 if swiglu else rows


# ----------------------------------------------------------------------------------------------------------------------
# bite: faults applied to the reference side
# ----------------------------------------------------------------------------------------------------------------------
def _differs(true_set: Tuple[torch.Tensor, torch.Tensor], pert2: torch.Tensor, swiglu: bool) -> bool:
    """A kernel computing `pert2` would fail the comparison somewhere: no admissible output of the faulty sums lies in the
    admissible set of the true ones."""
    lo, hi = true_set
    plo, phi = expected(pert2, swiglu)
    return bool((~member(plo, lo, hi) & ~member(phi, lo, hi)).any())


def _partial2(op: Operands, m_rows: int, lo: int, hi: int) -> torch.Tensor:
    return op.xop2[:m_rows, lo:hi] @ op.w[:, lo:hi].long().t()


def bites(op: Operands, m_rows: int, m_pad: int, ranges: Sequence[Tuple[int, int]], step: int, chunk: int, feats: int,
          swiglu: bool, pad: float) -> Dict[str, bool]:
    """Each class of fault, applied to the exact reference of the case's m_rows rows: True where the faulty result
    differs from the true one (for SwiGLU: falls outside the admissible set).  The 24 non-zeros of a sparse row cannot
    reach all of up to 304 k-steps, so the K faults are aimed where the case has data -- one target in EVERY range of
    `ranges`, which must exist (that is the coverage the stratified draw gives):
      zero_step   the `step`-column k-step that holds a non-zero of row 0 of the sparse operand, in every K range;
      move_split  at every inner boundary, the nearest `chunk` on either side with a non-zero partial sum, counted twice
                  and dropped;
      swap_rows   every adjacent pair of weight rows inside the first and the last tile (all of them for m_rows > 1; a
                  single token row cannot tell every pair apart: there at least one pair per tile);
      swap_gate_up  the gate and up halves of the first and of the last tile;
      pad_row     padding row m_rows (all `pad`) taken for token row m_rows - 1."""
    # Faults are judged element by element, so one that shows in the first rows shows in every case that has them: the K
    # faults are judged on token row 0 alone (every case has it), the row faults on the first min(m_rows, 15) rows, and
    # both are worked out once per operand set.
    memo = op.__dict__.setdefault("_memo", {})
    key = (tuple(ranges), step, chunk, feats, swiglu, min(m_rows, 15))
    if key not in memo:
        memo[key] = _shared_bites(op, min(m_rows, 15), ranges, step, chunk, feats, swiglu)
    out = dict(memo[key])
    true2 = op.ref2[:m_rows]
    true_set = expected(true2[m_rows - 1:], swiglu)
    if m_rows < m_pad:
        if pad != pad:
            out["pad_row"] = True                            # a NaN row equals nothing
        else:
            pert = (2 * pad * op.w.double().sum(1)).long()[None]
            out["pad_row"] = _differs(true_set, pert, swiglu)
    return out


def _shared_bites(op: Operands, m_rows: int, ranges, step: int, chunk: int, feats: int, swiglu: bool) -> Dict[str, bool]:
    k_rows = 1
    true2 = op.ref2[:k_rows]
    n = true2.shape[1]
    true_set = expected(true2, swiglu)
    out: Dict[str, bool] = {}
    ok = True
    for lo, hi in ranges:
        hit = [int(c) for c in op.sparse_row0 if lo <= int(c) < hi]
        ok = ok and bool(hit)
        if hit:
            s0 = hit[0] // step * step
            ok = ok and _differs(true_set, true2 - _partial2(op, k_rows, s0, s0 + step), swiglu)
    out["zero_step"] = ok
    ok = True
    for (lo, hi), (lo2, hi2) in zip(ranges, ranges[1:]):
        assert hi == lo2
        before = next((c for c in range(hi - chunk, lo - 1, -chunk) if bool(_partial2(op, k_rows, c, c + chunk).any())), None)
        after = next((c for c in range(lo2, hi2, chunk) if bool(_partial2(op, k_rows, c, c + chunk).any())), None)
        ok = ok and before is not None and after is not None
        for c in (before, after):
            if c is not None:
                part = _partial2(op, k_rows, c, c + chunk)
                ok = ok and _differs(true_set, true2 + part, swiglu) and _differs(true_set, true2 - part, swiglu)
    out["move_split"] = ok
    true2 = op.ref2[:m_rows]
    width = n // 2 if swiglu else n
    swaps, halves = [], []
    for t in sorted({0, width // feats - 1}):
        idx = list(range(feats * t, feats * (t + 1)))
        if swiglu:
            idx += [width + j for j in idx]
        sub = true2[:, idx]                                  # the tile's rows: [gate feats | up feats] or [feats]
        sub_set = expected(sub, swiglu)
        found = []
        for j in [j for j in range(len(idx) - 1) if j != feats - 1]:
            pert = sub.clone()
            pert[:, [j, j + 1]] = sub[:, [j + 1, j]]
            found.append(_differs(sub_set, pert, swiglu))
        swaps.append(all(found) if m_rows > 1 else any(found))
        if swiglu:
            halves.append(_differs(sub_set, torch.cat([sub[:, feats:], sub[:, :feats]], dim=1), True))
    out["swap_rows"] = all(swaps)
    if swiglu:
        out["swap_gate_up"] = all(halves)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the RMSNorm prologue, emulated as documented
# ----------------------------------------------------------------------------------------------------------------------
def prologue_operand(x: torch.Tensor, delta: torch.Tensor, norm_w: torch.Tensor, rstd_error: float = 0.0) -> torch.Tensor:
    """X = norm_w * bf16((x + delta) * rsqrt(mean((x + delta)^2) + eps)), the sum rounded to bf16 first; fp64 where the
    kernel has fp32, `rstd_error` a relative error put on the reciprocal square root."""
    s = (x.double() + delta.double()).float().to(BF).double()
    rstd = (1.0 + rstd_error) / torch.sqrt((s * s).mean(1, keepdim=True) + EPS)
    normed = (s * rstd).float().to(BF).double()
    return (norm_w.double() * normed).float().to(BF)
