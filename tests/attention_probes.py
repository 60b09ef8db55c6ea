"""One-key probes for the attention kernels: construction, fp32 references and guards, all on the CPU (this module never
loads the native library; tests/test_attention_probes_host.py proves every guard without a GPU, and
tests/test_attention_probes_gpu.py runs the same cases through the kernels).

Random-normal q/k/v gives a nearly flat softmax: one key weighs ~1/n and a wrong key hides below any tolerance.  Here
every token (and kv head) gets a random sign vector s[t] in {+-1}^128 as its key, and a query is 4 * s[target]:

  selection probe  the target is a key the row may see.  It scores 4 * 128 / sqrt(128) = 45.3 nats, every other key
                   4 * (s . s') / sqrt(128); with the off-target softmax mass <= 2^-20 (asserted from the reference:
                   `selection_mass`) the kernels' output is V[target] to the bit: the running row maximum is the
                   target's score, its P is exp2(0) = 1 (the pair kernel: exp2 of an fma residual <= 2^-18), whatever
                   was accumulated before it is rescaled by <= 2^-35, l = 1 + eps, and V (0.5 <= |v| < 2, bf16) moves
                   by a relative 2^-18 at most against half a bf16 ulp of 2^-9.
  lure probe       the target is a key the row must NOT see.  The visible keys score as noise (an ordinary soft mixture,
                   compared with the fp32 reference at atol = rtol = 2e-2); were the key let in it would take the whole
                   row: the reference with the mask widened by that key differs from the right one by more than ten
                   times the bar (asserted: `lure_guard`), with the key's real V row and with the zero V^T pad slot a
                   key behind a segment's end has.

The fused kernels of <= 32 tokens normalise and rotate q and k themselves: raw q = s[target], raw k = s (RMS 1), the
norm weights are the gain (a bf16-exact constant), and the same sign vector on both sides keeps the slow RoPE dimensions
aligned at any distance <= 31; their selection bound is 2^-24 (the bf16 rounding of the rotated q and k moves a score
by about a nat at most)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

D = 128
BF = torch.bfloat16
SCALE = 1.0 / math.sqrt(D)
TAIL = 32                     # rows qkv extends past T
ATOL = RTOL = 2e-2            # the bar of test_attention_property_random_lengths_and_groups
SELECTION_MASS = 2.0 ** -20
SMALL_SELECTION_MASS = 2.0 ** -24
ROPE_THETA = 1_000_000.0
EPS = 1e-6
Q_GAIN = 4.0
SMALL_SELECT_GAINS = (4.0, 4.0)   # (q norm weight, k norm weight) of the fused kernels' selection probes
# Lure probes of the fused kernels: gain 1.  The kernels round the normalised, rotated q and k to bf16 (relative 2^-9 per
# element, on both sides), which the fp32 reference does not: a score moves by about 2^-8 of the score scale.  At a gain
# product of 4 (visible keys 4 nats rms, as in the plain construction) that shifts the weights of two competing visible
# keys by percents of |v| <= 2, more than the comparison's 2e-2; at gain 1 the visible keys are 1 nat rms, the roundings
# move an output by a few 1e-3, and the lure (128 * ~0.8 / sqrt(128) = 9 nats) still takes a widened row (the guard).
SMALL_LURE_GAINS = (1.0, 1.0)


# ----------------------------------------------------------------------------------------------------------------------
# layout of a packed batch: who may see whom, in rows of qkv
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Layout:
    lens: List[int]
    parent: List[int]            # -1: a root
    cu: np.ndarray               # [B + 1]
    seq_of: np.ndarray           # [T]
    local: np.ndarray            # [T] index inside the own segment
    allowed: torch.Tensor        # bool [T, T + TAIL]: row i may attend to row j of qkv

    @property
    def t(self) -> int:
        return int(self.cu[-1])

    @staticmethod
    def build(lens: Sequence[int], parent: Optional[Sequence[int]] = None) -> "Layout":
        lens = [int(n) for n in lens]
        parent = [-1] * len(lens) if parent is None else [int(p) for p in parent]
        cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        t = int(cu[-1])
        seq_of = np.repeat(np.arange(len(lens)), lens)
        local = np.arange(t) - cu[seq_of]
        allowed = torch.zeros(t, t + TAIL, dtype=torch.bool)
        for b, n in enumerate(lens):
            lo = int(cu[b])
            allowed[lo:lo + n, lo:lo + n] = torch.ones(n, n).tril().bool()
            if parent[b] >= 0:
                allowed[lo:lo + n, int(cu[parent[b]]):int(cu[parent[b] + 1])] = True
        return Layout(lens, parent, cu, seq_of, local, allowed)


# ----------------------------------------------------------------------------------------------------------------------
# target maps: per name, the row of qkv every row of the batch aims at
# ----------------------------------------------------------------------------------------------------------------------
PLAIN_MAPS = ("diag", "prev", "first", "slot", "back32", "back64", "edge", "below_edge", "random")
SMALL_MAPS = ("diag", "prev", "first", "back16", "random", "edge16", "below_edge16")
CHILD_MAPS = ("parent_mod", "parent_last", "own_first", "own_diag", "own_back32")
PLAIN_LURES = ("next", "tile_above", "next_segment")
SMALL_LURES = ("prev_segment_last", "next_segment_first", "next_in_batch", "block_above")
PREFIXED_LURES = ("child_key|behind_parent", "next|sibling", "tile_above|other_root", "last_child_first|next",
                  "next|tile_above")


def _own_key(lay: Layout, name: str, rng: np.random.Generator) -> np.ndarray:
    """A visible key of the row's own segment, as an index inside the segment."""
    i = lay.local
    if name in ("diag", "own_diag"):
        return i.copy()
    if name == "prev":
        return np.maximum(i - 1, 0)
    if name in ("first", "own_first"):
        return np.zeros_like(i)
    if name == "slot":
        return i % 32
    if name in ("back32", "own_back32"):
        return np.maximum(i - 32, 0)
    if name == "back64":
        return np.maximum(i - 64, 0)
    if name == "back16":
        return np.maximum(i - 16, 0)
    if name == "edge":
        return 32 * (i // 32)
    if name == "below_edge":
        return np.maximum(32 * (i // 32) - 1, 0)
    if name == "edge16":
        return 16 * (i // 16)
    if name == "below_edge16":
        return np.maximum(16 * (i // 16) - 1, 0)
    if name == "random":
        return rng.integers(0, i + 1)
    raise KeyError(name)


def selection_targets(lay: Layout, names: Sequence[str], seed: int) -> np.ndarray:
    """[T, len(names)] rows of qkv: names[h] is head h's map.  A prefixed map is 'root map|child map'."""
    rng = np.random.default_rng(seed)
    par = np.asarray(lay.parent)[lay.seq_of]
    is_child = par >= 0
    p_begin, p_len = lay.cu[np.maximum(par, 0)], np.asarray(lay.lens)[np.maximum(par, 0)]
    out = np.empty((lay.t, len(names)), dtype=np.int64)
    for h, name in enumerate(names):
        root_name, _, child_name = name.partition("|")
        tgt = lay.cu[lay.seq_of] + _own_key(lay, root_name, rng)
        if child_name:
            if child_name == "parent_mod":
                c = p_begin + lay.local % np.maximum(p_len, 1)
            elif child_name == "parent_last":
                c = p_begin + p_len - 1
            else:
                c = lay.cu[lay.seq_of] + _own_key(lay, child_name, rng)
            tgt = np.where(is_child, c, tgt)
        out[:, h] = tgt
    rows = torch.arange(lay.t)
    for h in range(len(names)):
        assert bool(lay.allowed[rows, torch.from_numpy(out[:, h])].all()), names[h]
    return out


def lure_targets(lay: Layout, names: Sequence[str]) -> np.ndarray:
    """[T, len(names)] rows of qkv no row may see (asserted).  'next' = the row behind (a later key, the next segment's
    first row or the first row past T), 'tile_above' = 32 rows on (the slot of the pair kernel's second tile),
    'block_above' = 16 rows on, 'next_segment' = the first row behind the own segment.  Where a named key does not
    exist for a row (no previous segment, no child, a row past the batch) the row falls back to another forbidden key."""
    t, cu, seq = lay.t, lay.cu, lay.seq_of
    g = np.arange(t)
    nseq = len(lay.lens)
    par_of = np.asarray(lay.parent)
    par = par_of[seq]
    is_child = par >= 0
    lens = np.asarray(lay.lens)
    nxt = g + 1
    prev_last = np.where(seq > 0, cu[seq] - 1, cu[seq + 1])           # first segment: the next one's first row
    next_first = cu[seq + 1]
    children = [np.nonzero(par_of == b)[0] for b in range(nseq)]
    roots = [b for b in range(nseq) if par_of[b] < 0]

    def key_of(b, i):   # key i mod len of segment b
        return cu[b] + i % lens[b]

    def one(name):
        if name == "next":
            return nxt
        if name == "next_in_batch":
            return np.where(nxt < t, nxt, prev_last)
        if name == "tile_above":
            return g + 32
        if name == "block_above":
            return np.where(g + 16 < t, g + 16, prev_last)
        if name == "next_segment":
            return next_first
        if name == "prev_segment_last":
            return np.where(prev_last < t, prev_last, nxt)
        if name == "next_segment_first":
            return np.where(next_first < t, next_first, prev_last)
        if name in ("child_key", "last_child_first"):                 # root rows only
            f = nxt.copy()
            for b in roots:
                if len(children[b]):
                    rows = slice(int(cu[b]), int(cu[b + 1]))
                    f[rows] = key_of(children[b][0], lay.local[rows]) if name == "child_key" else cu[children[b][-1]]
            return f
        if name == "behind_parent":                                   # child rows only
            f = nxt.copy()
            for b in range(nseq):
                if par_of[b] >= 0:
                    behind = int(cu[par_of[b] + 1])
                    rows = slice(int(cu[b]), int(cu[b + 1]))
                    # directly behind its parent the row behind the parent is the child's own first key: visible
                    f[rows] = behind if behind != int(cu[b]) else key_of(roots[1], lay.local[rows])
            return f
        if name == "sibling":
            f = nxt.copy()
            for b in range(nseq):
                if par_of[b] >= 0:
                    sib = [c for c in children[par_of[b]] if c != b]
                    if not sib:                                       # an only child: a child of another root
                        sib = [c for c in range(nseq) if par_of[c] >= 0 and c != b]
                    rows = slice(int(cu[b]), int(cu[b + 1]))
                    f[rows] = key_of(sib[-1], lay.local[rows])
            return f
        if name == "other_root":
            f = nxt.copy()
            for b in range(nseq):
                if par_of[b] >= 0:
                    other = [r for r in roots if r != par_of[b] and not len(children[r])][0]
                    rows = slice(int(cu[b]), int(cu[b + 1]))
                    f[rows] = key_of(other, lay.local[rows])
            return f
        raise KeyError(name)

    out = np.empty((t, len(names)), dtype=np.int64)
    rows = torch.arange(t)
    for h, name in enumerate(names):
        root_name, _, child_name = name.partition("|")
        f = one(root_name)
        if child_name:
            f = np.where(is_child, one(child_name), f)
        assert (f >= 0).all() and (f < t + TAIL).all(), name
        assert not bool(lay.allowed[rows, torch.from_numpy(f)].any()), name
        out[:, h] = f
    return out


def head_maps(maps: Sequence[str], hq: int) -> List[List[str]]:
    """The launches of one case: every map at least once, head h of launch n takes maps[(n * hq + h) % len(maps)] -- the
    heads of a GQA group (<= len(maps) consecutive heads) never share a map."""
    return [[maps[(n * hq + h) % len(maps)] for h in range(hq)] for n in range(-(-len(maps) // hq))]


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def build_qkv(t: int, hq: int, hkv: int, tgt: np.ndarray, seed: int, q_gain: float = Q_GAIN, tail: str = "nan") -> torch.Tensor:
    """bf16 [T + TAIL, (hq + 2 hkv) * 128]: K[t] = s[t], V random with 0.5 <= |v| < 2, Q[i, h] = q_gain * s[tgt[i, h]].
    tail 'nan': the rows past T hold NaN; 'keys': they hold sign-vector keys and finite V like every other row."""
    g = torch.Generator().manual_seed(seed)
    rows = t + TAIL
    s = (torch.randint(0, 2, (rows, hkv, D), generator=g) * 2 - 1).float()
    mant = torch.randint(0, 128, (rows, hkv, D), generator=g).float()
    expo = torch.randint(-1, 1, (rows, hkv, D), generator=g).float()
    sign = (torch.randint(0, 2, (rows, hkv, D), generator=g) * 2 - 1).float()
    v = sign * torch.exp2(expo) * (1 + mant / 128)                     # bf16-exact, 0.5 <= |v| < 2
    q = torch.zeros(rows, hq, D)
    grp = hq // hkv
    idx = torch.from_numpy(tgt)
    for h in range(hq):
        q[:t, h] = q_gain * s[idx[:, h], h // grp]
    qkv = torch.cat([q.reshape(rows, -1), s.reshape(rows, -1), v.reshape(rows, -1)], dim=1)
    if tail == "nan":
        qkv[t:] = float("nan")
    else:
        assert tail == "keys"
    out = qkv.to(BF)
    assert torch.equal(out[:t].float(), qkv[:t])                      # every value is exact in bf16
    return out


def split(qkv: torch.Tensor, hq: int, hkv: int, t: Optional[int] = None):
    """fp32 views q [t, hq, 128] (the first t rows), k and v [rows, hkv, 128] of a fused qkv tensor."""
    f = qkv.float().cpu()
    t = f.shape[0] if t is None else t
    return (f[:t, : hq * D].reshape(t, hq, D), f[:, hq * D: (hq + hkv) * D].reshape(-1, hkv, D),
            f[:, (hq + hkv) * D:].reshape(-1, hkv, D))


def rope_ref(x: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """x [T, H, 128] fp32, rotate-half form (the arithmetic of test_encoder_gpu._rope_ref)."""
    half = D // 2
    inv = 1.0 / (ROPE_THETA ** (torch.arange(0, half, dtype=torch.float32) * 2.0 / D))
    ang = pos.float()[:, None] * inv[None, :]
    cos, sin = torch.cat([ang.cos(), ang.cos()], -1)[:, None, :], torch.cat([ang.sin(), ang.sin()], -1)[:, None, :]
    rot = torch.cat([-x[..., half:], x[..., :half]], -1)
    return x * cos + rot * sin


def norm_rope_ref(x: torch.Tensor, gain: float, pos: torch.Tensor) -> torch.Tensor:
    """fp32 per-head RMSNorm with the constant weight `gain`, then RoPE."""
    return rope_ref(x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * gain, pos)


# ----------------------------------------------------------------------------------------------------------------------
# references and guards
# ----------------------------------------------------------------------------------------------------------------------
def _heads(q, k, v, allowed, extra, dtype):
    """Per head: (h, softmax [T, R] under the mask (widened by extra[:, h] when given), V [R, 128] with the rows nobody may
    see zeroed so that a NaN there stays out of the product)."""
    t, hq, _ = q.shape
    grp = hq // k.shape[1]
    rows = torch.arange(t)
    r = k.shape[0]
    allowed = allowed[:, :r]
    for h in range(hq):
        mask = allowed
        if extra is not None:
            assert not bool(allowed[rows, extra[:, h]].any())
            mask = allowed.clone()
            mask[rows, extra[:, h]] = True
        sc = (q[:, h].to(dtype) @ k[:, h // grp].to(dtype).T) * SCALE
        p = torch.softmax(sc.masked_fill(~mask, float("-inf")), dim=-1)
        vv = v[:, h // grp].to(dtype)
        yield h, p, torch.where(mask.any(0)[:, None], vv, torch.zeros_like(vv))


def reference(q, k, v, allowed) -> torch.Tensor:
    """fp32 masked softmax attention, GQA: out [T, hq, 128]."""
    out = torch.empty(q.shape, dtype=torch.float32)
    for h, p, vv in _heads(q, k, v, allowed, None, torch.float32):
        out[:, h] = p @ vv
    return out


def selection_mass(q, k, v, allowed, tgt: np.ndarray) -> torch.Tensor:
    """[T, hq] softmax mass of every key but the target (float64 softmax of the given q and k)."""
    idx = torch.from_numpy(tgt)
    rows = torch.arange(q.shape[0])
    mass = torch.empty(q.shape[0], q.shape[1], dtype=torch.float64)
    for h, p, _ in _heads(q, k, v, allowed, None, torch.float64):
        p[rows, idx[:, h]] = 0.0
        mass[:, h] = p.sum(-1)
    return mass


def lure_guard(q, k, v, allowed, forb: np.ndarray, ref: torch.Tensor) -> torch.Tensor:
    """bool [T, hq]: the reference with row i's mask widened by forb[i, h] differs from `ref` by more than
    10 * (ATOL + RTOL * |ref|) in at least one element (a non-finite leak counts as different), with the lure's own V row
    and with a zero V^T slot in its place."""
    idx = torch.from_numpy(forb)
    rows = torch.arange(q.shape[0])
    grp = q.shape[1] // k.shape[1]
    ok = torch.empty(q.shape[0], q.shape[1], dtype=torch.bool)
    bar = 10.0 * (ATOL + RTOL * ref.abs())
    for h, p, vv in _heads(q, k, v, allowed, idx, torch.float32):
        wide = p @ vv
        pad = wide - p[rows, idx[:, h]][:, None] * vv[idx[:, h]]
        good = torch.ones(q.shape[0], dtype=torch.bool)
        for leak in (wide, pad):
            good &= (((leak - ref[:, h]).abs() > bar[:, h]) | ~torch.isfinite(leak)).any(-1)
        ok[:, h] = good
    return ok


# ----------------------------------------------------------------------------------------------------------------------
# the cases (shared by the host and the GPU file)
# ----------------------------------------------------------------------------------------------------------------------
RAGGED = [1, 33, 64, 200, 97, 31]     # q blocks with 1 .. 7 key tiles: full and half last pairs, ragged ends


@dataclass(frozen=True)
class AttnCase:
    name: str
    lens: tuple
    hq: int
    hkv: int
    single: bool = False              # CRAG_ATTN_SINGLE=1: attention_kernel<4, false> instead of the pair kernel
    seed: int = 0


ATTENTION_SELECT = [
    AttnCase("g1", tuple(RAGGED), 4, 4, seed=11),
    AttnCase("g2", tuple(RAGGED), 4, 2, seed=12),
    AttnCase("g4-pair", tuple(RAGGED), 8, 2, seed=13),
    AttnCase("g8-pair", tuple(RAGGED), 8, 1, seed=14),
    AttnCase("g4-pair-32x8", tuple(RAGGED), 32, 8, seed=15),
    AttnCase("g4-single", tuple(RAGGED), 8, 2, single=True, seed=16),
    AttnCase("g4-pair-long", (1100,), 8, 2, seed=17),
]
ATTENTION_LURE = [AttnCase(f"{c.name}-{tag}", lens, c.hq, c.hkv, c.single, c.seed + 100 * (1 + n))
                  for c in ATTENTION_SELECT[:6] for n, (tag, lens) in enumerate((("3seq", (33, 64, 31)), ("ragged", tuple(RAGGED))))]


@dataclass(frozen=True)
class PrefixedCase:
    name: str
    plen: int
    hq: int
    hkv: int
    seed: int

    @property
    def lens(self):   # root, unrelated root, three children of the root, a second root of the root's length, its child
        return [self.plen, 45, 1, 17, 70, self.plen, 40]

    @property
    def parent(self):
        return [-1, -1, 0, 0, 0, -1, 5]


PREFIXED = [PrefixedCase(f"g{hq // hkv}-p{plen}", plen, hq, hkv, 1000 + 10 * plen + hq)
            for hq, hkv in ((4, 2), (8, 2)) for plen in (1, 31, 32, 33, 95)]
PREFIXED_SELECT_MAPS = tuple(f"{PLAIN_MAPS[n]}|{CHILD_MAPS[n % len(CHILD_MAPS)]}" for n in range(len(PLAIN_MAPS)))

SMALL_HEADS = (32, 8)
SMALL_LENS = [[16], [32], [7, 9], [3, 20, 9], [1, 1, 1, 1], [16, 3, 9, 16, 1, 12, 7, 15], [2] * 70]
SMALL_LURE_LENS = [[7, 9], [3, 20, 9], [16, 3, 9, 16, 1, 12, 7, 15]]


def small_seed(lens: Sequence[int], lure: bool = False) -> int:
    return 7 * sum(lens) + len(lens) + (500 if lure else 0)


def small_id(lens: Sequence[int]) -> str:
    return "x".join(str(n) for n in lens) if len(lens) <= 8 else f"{lens[0]}x{len(lens)}"


def small_inputs(lens: Sequence[int], lure: bool):
    """(layout, targets [T, hq], raw qkv bf16 [T + TAIL, width] (q = s[target], k = s: before norm and RoPE), gains)."""
    hq, hkv = SMALL_HEADS
    lay = Layout.build(lens)
    if lure:
        tgt = lure_targets(lay, head_maps(SMALL_LURES, hq)[0])
        assert (tgt < lay.t).all()                                     # these kernels read no row past T
    else:
        tgt = selection_targets(lay, head_maps(SMALL_MAPS, hq)[0], small_seed(lens))
    qkv = build_qkv(lay.t, hq, hkv, tgt, small_seed(lens, lure), q_gain=1.0)
    return lay, tgt, qkv, (SMALL_LURE_GAINS if lure else SMALL_SELECT_GAINS)


def small_qkv_ref(lay: Layout, qkv: torch.Tensor, gains):
    """fp32 q, k after norm -> RoPE and v, over the T real rows."""
    hq, hkv = SMALL_HEADS
    q, k, v = split(qkv[:lay.t], hq, hkv)
    pos = torch.from_numpy(lay.local)
    return norm_rope_ref(q, gains[0], pos), norm_rope_ref(k, gains[1], pos), v


def launches(lens, parent, hq: int, hkv: int, maps: Sequence[str], seed: int, lure: bool):
    """The launches of one case of the tiled kernels: (layout, the heads' map names, targets [T, hq], qkv).  A lure case
    runs every launch twice: the rows past T as NaN, and as keys with finite V."""
    lay = Layout.build(lens, parent)
    for n, names in enumerate(head_maps(maps, hq)):
        tgt = lure_targets(lay, names) if lure else selection_targets(lay, names, seed + n)
        for tail in (("nan", "keys") if lure else ("nan",)):
            yield lay, names, tgt, build_qkv(lay.t, hq, hkv, tgt, seed + n, tail=tail)
