"""Exact probes and bf16-chain references for the encoder's row operators and its two heads (embed_gather_kernel,
rmsnorm_kernel, qk_norm_rope_kernel / qk_rope_vt_kernel / kv_append_row through norm_rope_chunk, swiglu_kernel,
pool_normalize_kernel, rerank_head_kernel, lm_head_kernel + lm_argmax_kernel): construction, references and case lists,
all on the CPU (this module never loads the native library; tests/test_row_probes_host.py proves what the comparisons
rest on without a GPU, tests/test_row_probes_gpu.py runs the same inputs through the kernels).

Two kinds of check:

  chain check   random rows against a CHAIN REFERENCE: the operator in fp64, rounded to bf16 exactly where the kernels
                document a rounding (the residual sum, the normed element before the weight product, the weighted
                element, the cos/sin table, silu before the product with up).  check_chain asks two things: every element
                within MAX_ULPS = 2 bf16 steps, and at most MAX_SHARE = 1 % of the elements with other bits.  These are
                conditions, not measurements: an fp32 chain differs from the fp64 one in well under 0.1 % of the bits,
                also with its reciprocal square root off by 4 fp32 ulps (asserted on the host), while a dropped rounding
                changes a quarter of them.

  exact probe   a row (or head vector) whose elements are all +-C, C a power of two >= 0.5: the mean square is C^2
                exactly, C * rsqrt(C^2 + 1e-6) rounds to exactly 1.0 in bf16 for any rsqrt within a few fp32 ulps, so the
                normed element is +-1 and the output +-w[i] bit for bit -- or +-w[i] times an exactly representable table
                value.  w[i] has bit pattern 0x3000 + i (distinct positive normals), row r carries sign = bit r of the
                element index (row 13: all positive), so every index is identified by value and by its signature across
                the rows: a wrong chunk, lane, weight vector or stride changes bits."""
from __future__ import annotations

import math
import zlib
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import torch

import gemm_probes as gp

BF = torch.bfloat16
F64 = torch.float64
F32 = torch.float32
EPS = 1e-6
NAN = float("nan")
MAX_ULPS = 2
MAX_SHARE = 0.01
FAR = 1 << 17                                   # bf16_ulps between a NaN and a number
HIDDEN_EDGES = (8, 264, 2048, 2056, 2560, 8192)  # one chunk; 33 chunks; one full trip; one chunk more; the 4B width; the maximum
CHAIN_HIDDEN = (264, 2560, 8192)
CHAIN_SCALES = (3.0, 1.0, 2e-3)                 # at 2e-3 the mean square is 4e-6: eps decides every bit
CHAIN_ROWS = 16
PROBE_C = (1024.0, 0.5)
N_SIGNS = 14                                    # 13 index bits (hidden <= 8192) and the all-positive row
TINY = 2.0 ** -126                              # the smallest normal of bf16 and of fp32


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ----------------------------------------------------------------------------------------------------------------------
# bf16: rounding from fp64, bits, distances
# ----------------------------------------------------------------------------------------------------------------------
def to_bf16(x: torch.Tensor) -> torch.Tensor:
    """Round to nearest even.  From fp64 the detour over fp32 can round twice: the nearer of the candidate's two bf16
    neighbours wins (a tie in fp64 is a tie in fp32, which the cast already broke to even)."""
    if x.dtype != F64:
        return x.to(BF)
    best = x.float().to(BF)
    fin = torch.isfinite(x) & torch.isfinite(best.float())
    for cand in (gp._bf16_step(best, up=False), gp._bf16_step(best, up=True)):
        closer = (cand.double() - x).abs() < (best.double() - x).abs()
        best = torch.where(closer & fin & torch.isfinite(cand.float()), cand, best)
    return best


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


def from_bits(b: torch.Tensor) -> torch.Tensor:
    return b.to(torch.int16).view(BF)


def _ordered(t: torch.Tensor) -> torch.Tensor:
    b = bits(t).to(torch.int32) & 0xFFFF
    return torch.where(b < 0x8000, b, 0x8000 - b)           # -0 and +0 share 0, negatives run downwards


def bf16_ulps(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """Distance in ordered-integer space (int32); NaN matches only NaN (0), a NaN against a number is FAR."""
    gn, wn = got != got, want != want
    d = (_ordered(got) - _ordered(want)).abs()
    d = torch.where(gn & wn, torch.zeros_like(d), d)
    return torch.where(gn ^ wn, torch.full_like(d, FAR), d)


def same_bits(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """Equal bit patterns, NaN matching NaN."""
    return (bits(got) == bits(want)) | ((got != got) & (want != want))


def chain_stats(got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """[largest distance, number of elements whose bits differ, number of elements] (int64, on the inputs' device)."""
    assert got.shape == want.shape and got.dtype == BF and want.dtype == BF
    return torch.stack([bf16_ulps(got, want).max().long(), (~same_bits(got, want)).sum(),
                        torch.tensor(got.numel(), device=got.device)])


def check_chain(got: torch.Tensor, want: torch.Tensor, max_ulps: int = MAX_ULPS, max_share: float = MAX_SHARE,
                label: str = "") -> float:
    """Every element within max_ulps and at most max_share of them with other bits; returns the measured share."""
    worst, differ, n = chain_stats(got, want).tolist()
    share = differ / n
    assert worst <= max_ulps, f"{label}: an element is {worst} bf16 steps from the chain reference (bound {max_ulps})"
    assert share <= max_share, f"{label}: {share:.4%} of the bits differ from the chain reference (cap {max_share:.2%})"
    return share


def fails_chain(got: torch.Tensor, want: torch.Tensor, max_ulps: int = MAX_ULPS, max_share: float = MAX_SHARE) -> bool:
    try:
        check_chain(got, want, max_ulps, max_share)
    except AssertionError:
        return True
    return False


# ----------------------------------------------------------------------------------------------------------------------
# chain references (dtype fp64: the reference; dtype fp32: the stand-in for a kernel that the host file perturbs)
# ----------------------------------------------------------------------------------------------------------------------
def _eps(eps: float) -> float:
    return float(torch.tensor(eps, dtype=F32))               # the kernels take eps as a float


def rmsnorm_chain(x, w, eps, residual=None, *, dtype=F64, rstd_scale: float = 1.0, inner: bool = True):
    """(out, residual_out): s = bf16(x + residual); out = bf16(w * bf16(s * rsqrt(mean(s^2) + eps))), over the last
    dimension.  inner=False drops the rounding of the normed element; rstd_scale multiplies the reciprocal root."""
    s, res = x.to(dtype), None
    if residual is not None:
        res = to_bf16(s + residual.to(dtype))
        s = res.to(dtype)
    ms = (s * s).mean(-1, keepdim=True) + torch.tensor(_eps(eps), dtype=dtype)
    rstd = (torch.rsqrt(ms) if dtype == F32 else 1.0 / torch.sqrt(ms)) * torch.tensor(rstd_scale, dtype=dtype)
    normed = s * rstd
    if inner:
        normed = to_bf16(normed).to(dtype)
    return to_bf16(w.to(dtype) * normed), res


def rmsnorm_ref(x, w, eps, residual=None):
    return rmsnorm_chain(x, w, eps, residual)


def rope_rotate(n: torch.Tensor, table: torch.Tensor, positions: torch.Tensor, *, cast_table: bool = True,
                wrong_partner: bool = False) -> torch.Tensor:
    """bf16(n * cos + rotate_half(n) * sin) for normed head vectors n [T, H, 128] (fp64 or fp32), the table
    [max_pos, 64, 2] fp32 cast to bf16 as the model does, column i % 64 for element i; rotate_half(n)[i] = -n[i + 64]
    for i < 64 and n[i - 64] otherwise.  wrong_partner: the partner with the opposite sign."""
    cs = table[positions.long()]
    cs = (cs.to(BF) if cast_table else cs).to(n.dtype)
    c = torch.cat([cs[..., 0], cs[..., 0]], dim=-1)[:, None, :]
    s = torch.cat([cs[..., 1], cs[..., 1]], dim=-1)[:, None, :]
    rot = torch.cat([-n[..., 64:], n[..., :64]], dim=-1)
    if wrong_partner:
        rot = -rot
    return to_bf16(n * c + rot * s)


def norm_rope_chain(heads, w, table, positions, eps, *, dtype=F64, rstd_scale: float = 1.0, inner: bool = True,
                    cast_table: bool = True, wrong_partner: bool = False) -> torch.Tensor:
    """heads [T, H, 128] bf16, w [H, 128] (or [128]) bf16 -> [T, H, 128] bf16: per-head RMSNorm, then rope_rotate."""
    n = rmsnorm_chain(heads, w, eps, dtype=dtype, rstd_scale=rstd_scale, inner=inner)[0].to(dtype)
    return rope_rotate(n, table, positions, cast_table=cast_table, wrong_partner=wrong_partner)


def norm_rope_ref(head_vectors, w, cos_sin_table, positions, eps):
    return norm_rope_chain(head_vectors, w, cos_sin_table, positions, eps)


def head_weights(q_w: torch.Tensor, k_w: torch.Tensor, hq: int, hkv: int) -> torch.Tensor:
    """[hq + hkv, 128]: q_w for the q heads, k_w for the k heads."""
    return torch.cat([q_w[None].expand(hq, 128), k_w[None].expand(hkv, 128)])


def pooled_row_ref(hs, w, spans, mode: int, eps, delta=None, **kw) -> torch.Tensor:
    """[B, hidden] fp64: mode 0 the final RMSNorm (chain) of the last row of every span (+ delta), mode 1 the mean of the
    span's rows; an empty span gives zeros."""
    out = torch.zeros(len(spans), hs.shape[1], dtype=F64)
    for b, (t0, t1) in enumerate(spans):
        if t1 <= t0:
            continue
        if mode == 0:
            d = None if delta is None else delta[t1 - 1]
            out[b] = rmsnorm_chain(hs[t1 - 1], w, eps, d, **kw)[0].double()
        else:
            out[b] = hs[t0:t1].double().mean(0)
    return out


def pool_ref(hs, w, spans, out_dim: int, mode: int, eps, delta=None) -> torch.Tensor:
    """[B, out_dim] fp64: the pooled row's first out_dim elements over max(their L2 norm, 1e-12)."""
    row = pooled_row_ref(hs, w, spans, mode, eps, delta)[:, :out_dim]
    return row / row.norm(dim=1, keepdim=True).clamp_min(1e-12)


def head_ref(hs, w, eps, lm, delta=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(normed rows [n, hidden] bf16 by the chain, fp64 dots [n, V] with the rows of lm).  The products are summed
    element by element, so that an infinity or a NaN in lm behaves as IEEE says."""
    normed = rmsnorm_chain(hs, w, eps, delta)[0]
    return normed, (normed.double()[:, None, :] * lm.double()[None, :, :]).sum(-1)


def score_ref(yes: torch.Tensor, no: torch.Tensor) -> torch.Tensor:
    """exp(log_softmax([no, yes])[1]) = 1 / (1 + exp(no - yes)) in fp64."""
    return 1.0 / (1.0 + torch.exp(no.double() - yes.double()))


def argmax_ref(logits: torch.Tensor, banned: Sequence[int] = ()) -> List[int]:
    """Per row: the lowest id among the maxima, NaNs and banned ids left out; -1 when nothing is left."""
    out = []
    for row in logits:
        ok = ~torch.isnan(row)
        if len(banned):
            ok[torch.tensor(list(banned), dtype=torch.long)] = False
        if not bool(ok.any()):
            out.append(-1)
            continue
        top = row[ok].max()
        out.append(int(torch.nonzero(ok & (row == top))[0]))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# exact probes: patterns
# ----------------------------------------------------------------------------------------------------------------------
def pattern_weights(n: int, base: int = 0x3000) -> torch.Tensor:
    """bf16 [n] with bit pattern base + i: distinct positive normals (base 0x3000, n <= 8192: 2^-31 .. 2^32)."""
    b = base + torch.arange(n, dtype=torch.int32)
    assert int(b.max()) < 0x7F80 and int(b.min()) >= 0x0080
    return from_bits(b)


def signs(width: int, patterns: Sequence[int]) -> torch.Tensor:
    """[len(patterns), width] of +-1.0 (fp64): pattern p < 13 is negative where bit p of the element index is set,
    pattern 13 is all positive."""
    idx = torch.arange(width)
    rows = [torch.where(((idx >> p) & 1).bool() & (p < N_SIGNS - 1), -1.0, 1.0) for p in patterns]
    return torch.stack(rows).double()


def signed(w: torch.Tensor, sign: torch.Tensor) -> torch.Tensor:
    """+-w as bf16 (exact: a sign flip)."""
    return (w.double() * sign).float().to(BF)


def rmsnorm_probe(hidden: int, c: float, residual: bool) -> Dict[str, torch.Tensor]:
    """14 sign-signature rows of +-c.  residual: x = +-c/4 and residual_in = +-3c/4 of the same sign (the sum is exact).
    want_out = +-w, want_res = +-c."""
    sg = signs(hidden, range(N_SIGNS))
    w = pattern_weights(hidden)
    p = {"w": w, "want_out": signed(w, sg), "sum": (sg * c).float().to(BF)}
    if residual:
        p["x"], p["res_in"], p["want_res"] = (sg * c / 4).float().to(BF), (sg * 3 * c / 4).float().to(BF), p["sum"]
    else:
        p["x"] = p["sum"]
    return p


RSTD_SCALES = (1.0, 1 + 4 * 2.0 ** -23, 1 - 4 * 2.0 ** -23)
ROBUST_SHARE = MAX_SHARE / 10


def rstd_robust(x, w, residual=None) -> bool:
    """An fp32 chain, also with its reciprocal root off by 4 fp32 ulps either way, stays within MAX_ULPS of the fp64
    chain and differs from it in at most a tenth of the share cap.  All elements of a row meet ONE reciprocal root and
    bf16 inputs have 128 mantissas, so when that root lies within a few ulps of a mantissa's rounding boundary every
    element with that mantissa moves at once (~hidden / 128 of them: 0.5-1 % of the row).  The chain inputs are drawn so
    that no row sits there: what a kernel's rsqrt does in its last bits then cannot decide the comparison."""
    want = rmsnorm_chain(x, w, EPS, residual)[0]
    return not any(fails_chain(rmsnorm_chain(x, w, EPS, residual, dtype=F32, rstd_scale=s)[0], want, MAX_ULPS, ROBUST_SHARE)
                   for s in RSTD_SCALES)


def _robust_rows(key, rows: int, hidden: int, scale: float, with_res: bool):
    """(x, w, residual or None) random, the first of the seeds (key, attempt) that is rstd_robust (asserted again by the
    host file for what comes out)."""
    for attempt in range(16):
        g = _gen(key, hidden, scale, with_res, attempt)
        x = (torch.randn(rows, hidden, generator=g) * scale).to(BF)
        res = (torch.randn(rows, hidden, generator=g) * scale).to(BF) if with_res else None
        w = (1 + 0.1 * torch.randn(hidden, generator=g)).to(BF)
        if rstd_robust(x, w, res):
            return x, w, res
    raise AssertionError(f"no robust rows for {key} hidden={hidden} scale={scale}")


def rmsnorm_chain_cases() -> Iterator[Tuple[str, torch.Tensor, torch.Tensor, Optional[torch.Tensor]]]:
    """(label, x, w, residual or None): CHAIN_ROWS random rows at every CHAIN_HIDDEN x CHAIN_SCALES, with and without a
    residual."""
    for hidden in CHAIN_HIDDEN:
        for scale in CHAIN_SCALES:
            for with_res in (False, True):
                x, w, res = _robust_rows("rmsnorm", CHAIN_ROWS, hidden, scale, with_res)
                yield f"rmsnorm hidden={hidden} scale={scale} residual={int(with_res)}", x, w, res


# ----------------------------------------------------------------------------------------------------------------------
# q/k norm + RoPE
# ----------------------------------------------------------------------------------------------------------------------
ROPE_HEADS = ((1, 1), (4, 2), (16, 8), (20, 4), (32, 8))      # smallest; today's; switch at a group edge; switch inside
                                                              # the second trip; the 4B model, three trips
APPEND_HEADS = tuple(h for h in ROPE_HEADS if h[0] // h[1] in (2, 4) and h[0] % h[1] == 0)   # what decode / extend take
ROPE_TOKENS = (1, 5)
ROPE_MAX_POS = 16
ROPE_POSITIONS = {1: (ROPE_MAX_POS - 1,), 5: (ROPE_MAX_POS - 1, 0, 7, 3, 10)}
ROPE_TABLES = ("identity", "quarter", "poscol-cos", "poscol-sin", "cast", "cast-3")
Q_BASE, K_BASE = 0x3C00, 0x3D80                               # q_w in [0.0078, 0.0156), k_w in [0.0625, 0.125)


def rope_table(kind: str, max_pos: int = ROPE_MAX_POS) -> torch.Tensor:
    """[max_pos, 64, 2] fp32 (cos, sin)."""
    t = torch.zeros(max_pos, 64, 2)
    poscol = 2.0 ** -(torch.arange(max_pos) % 8).float()[:, None] * (1 + torch.arange(64).float() / 64)[None, :]
    if kind == "identity":
        t[..., 0] = 1.0
    elif kind == "quarter":
        t[..., 1] = 1.0
    elif kind == "poscol-cos":
        t[..., 0] = poscol
    elif kind == "poscol-sin":
        t[..., 1] = poscol
    elif kind == "cast":               # not a bf16 value; bf16(1 + 2^-10) = 1
        t[..., 0] = 1.0 + 2.0 ** -10
    elif kind == "cast-3":             # bf16(1 + 3 * 2^-10) = 1, and w * (1 + 3 * 2^-10) rounds away from w for many w
        t[..., 0] = 1.0 + 3 * 2.0 ** -10
    else:
        raise ValueError(kind)
    return t


def real_rope_table(max_pos: int) -> torch.Tensor:
    inv_freq = 1.0 / (1_000_000.0 ** (torch.arange(0, 64, dtype=F32) * 2.0 / 128))
    ang = torch.arange(max_pos, dtype=F32)[:, None] * inv_freq[None, :]
    return torch.stack([ang.cos(), ang.sin()], dim=-1).contiguous()


class RopeProbe:
    """n_tokens rows [q heads | k heads | v heads] of head vectors +-C (sign signature over the 128 elements, pattern
    (head + 3 token) % 8, C alternating 1024 / 0.5) with raw v columns of arbitrary bits, and what the q|k columns must
    hold afterwards: rope_rotate(+-w)."""

    def __init__(self, hq: int, hkv: int, n_tokens: int, kind: str, positions: Optional[Sequence[int]] = None):
        self.hq, self.hkv, self.n_tokens, self.kind = hq, hkv, n_tokens, kind
        heads = hq + hkv
        self.positions = torch.tensor(ROPE_POSITIONS[n_tokens] if positions is None else positions, dtype=torch.int32)
        assert self.positions.numel() == n_tokens and int(self.positions.max()) < ROPE_MAX_POS
        self.table = rope_table(kind)
        ones = kind.startswith("poscol")
        self.q_w = torch.ones(128, dtype=BF) if ones else pattern_weights(128, Q_BASE)
        self.k_w = torch.ones(128, dtype=BF) if ones else pattern_weights(128, K_BASE)
        t, h = torch.meshgrid(torch.arange(n_tokens), torch.arange(heads), indexing="ij")
        # (pattern 7 is all positive: no element index below 128 has bit 7)
        self.sign = signs(128, range(8)).index_select(0, ((h + 3 * t) % 8).flatten()).view(n_tokens, heads, 128)
        c = torch.tensor(PROBE_C, dtype=F64)[(h + t) % 2][..., None]
        self.heads = (self.sign * c).float().to(BF)                                   # [T, heads, 128]
        g = _gen("rope-v", hq, hkv, n_tokens)
        self.v = torch.randn(n_tokens, hkv * 128, generator=g).to(BF)
        self.qkv = torch.cat([self.heads.view(n_tokens, heads * 128), self.v], dim=1)
        self.w = head_weights(self.q_w, self.k_w, hq, hkv)
        self.want = rope_rotate(self.sign * self.w.double(), self.table, self.positions).view(n_tokens, heads * 128)

    def chain(self, **kw) -> torch.Tensor:
        return norm_rope_chain(self.heads, self.w, self.table, self.positions, EPS, **kw).view(self.n_tokens, -1)


def rope_probes(heads=ROPE_HEADS, positions=None) -> Iterator[RopeProbe]:
    """positions: {n_tokens: positions} instead of ROPE_POSITIONS."""
    for hq, hkv in heads:
        for n_tokens in ROPE_TOKENS:
            for kind in ROPE_TABLES:
                yield RopeProbe(hq, hkv, n_tokens, kind, None if positions is None else positions[n_tokens])


# The cache append: decode appends one row per sequence at position len of its slot, extend new_len rows at len.. .
# (slot, cached rows, new rows) per sequence; the positions that follow are 15 | 15, 0, 7, 3, 10 and 15 | 13, 14, 15, 0, 1.
APPEND_MAX_LEN = ROPE_MAX_POS
DECODE_SEQS = {1: ((4, 15, 1),), 5: ((3, 15, 1), (0, 0, 1), (6, 7, 1), (1, 3, 1), (7, 10, 1))}
EXTEND_SEQS = {1: ((4, 15, 1),), 5: ((2, 13, 3), (5, 0, 2))}


def append_positions(seqs) -> Dict[int, Tuple[int, ...]]:
    return {t: tuple(m + i for _, m, n in ss for i in range(n)) for t, ss in seqs.items()}


CHAIN_ROPE_TOKENS = 16
CHAIN_ROPE_MAX_POS = 64


def rope_robust(heads, w, table, pos) -> bool:
    """rstd_robust for norm + RoPE.  Here the distance bound needs it too: n * cos + rotate_half(n) * sin cancels for some
    elements, and where it does one bf16 step of n (which 4 ulps of the reciprocal root buy in ~0.01 % of the elements)
    is several steps of the much smaller result.  The inputs are drawn so that no such element decides the comparison."""
    want = norm_rope_chain(heads, w, table, pos, EPS)
    return not any(fails_chain(norm_rope_chain(heads, w, table, pos, EPS, dtype=F32, rstd_scale=s), want, MAX_ULPS,
                               ROBUST_SHARE) for s in RSTD_SCALES)


def rope_chain_case(hq: int, hkv: int):
    """(heads [16, hq + hkv, 128], v [16, hkv * 128], q_w, k_w, table, positions): random head vectors, the real table;
    the first seed that is rope_robust (asserted again by the host file)."""
    table = real_rope_table(CHAIN_ROPE_MAX_POS)
    for attempt in range(32):
        g = _gen("rope-chain", hq, hkv, attempt)
        heads = torch.randn(CHAIN_ROPE_TOKENS, hq + hkv, 128, generator=g).to(BF)
        v = torch.randn(CHAIN_ROPE_TOKENS, hkv * 128, generator=g).to(BF)
        q_w = (1 + 0.1 * torch.randn(128, generator=g)).to(BF)
        k_w = (1 + 0.1 * torch.randn(128, generator=g)).to(BF)
        pos = torch.randperm(CHAIN_ROPE_MAX_POS, generator=g)[:CHAIN_ROPE_TOKENS].to(torch.int32)
        pos[0], pos[1] = CHAIN_ROPE_MAX_POS - 1, 0
        if rope_robust(heads, head_weights(q_w, k_w, hq, hkv), table, pos):
            return heads, v, q_w, k_w, table, pos
    raise AssertionError(f"no robust head vectors for hq={hq} hkv={hkv}")


# ----------------------------------------------------------------------------------------------------------------------
# SwiGLU
# ----------------------------------------------------------------------------------------------------------------------
SWIGLU_UPS = (1.0, -3.0, 0.7421875)
SWIGLU_INTERS = (8, 264, 8192, 8200, 9728)
SWIGLU_ROWS = (1, 3)
GATE32_BITS = 0x4200


def all_gates() -> torch.Tensor:
    """All 65 536 bf16 bit patterns as 8 rows of 8192."""
    return from_bits(torch.arange(65536, dtype=torch.int32)).view(8, 8192)


def swiglu_exhaustive(up_value: float) -> Dict[str, torch.Tensor]:
    """For every gate pattern under one up value: `nan` where fp64 silu(gate) * up is NaN (NaN gates and -inf); the
    admissible pair (lo, hi) = swiglu_set; `exact` the member from the correctly rounded silu; `normal` where that silu
    is a normal bf16 number; `small` where the gate or its silu is below the normals, with `zero` the zero of the
    product's sign, which is accepted there as well."""
    gate = all_gates()
    g = gate.double()
    nan = torch.isnan(g) | (g == -math.inf)
    safe = torch.where(nan, torch.zeros_like(gate), gate)
    up = torch.full_like(gate, up_value)
    assert float(up[0, 0]) == up_value
    lo, hi = gp.swiglu_set(safe, up)
    sd = safe.double()
    silu = to_bf16(sd / (1.0 + torch.exp(-sd)))
    exact = (silu.float() * up.float()).to(BF)
    mag = silu.float().abs()
    normal = ~nan & (mag >= TINY) & torch.isfinite(mag)
    small = ~nan & ((sd.abs() < TINY) | (mag < TINY))
    negative = torch.signbit(sd) ^ (up_value < 0)
    zero = torch.where(negative, -torch.zeros_like(gate), torch.zeros_like(gate))
    return {"gate": gate, "up": up, "nan": nan, "lo": lo, "hi": hi, "exact": exact, "normal": normal, "small": small,
            "zero": zero}


def swiglu_selection(inter: int, rows: int) -> Dict[str, torch.Tensor]:
    """gate_up / want for the two selection probes.  "up": gate 32 (silu exactly 32) against up of distinct patterns, the
    output up * 2^5 (five exponent steps: bits + 0x280).  "gate": up 1 against gates of distinct patterns >= 32, the
    output the gate's bits (1 + exp(-g) is 1 in fp32 and in fp64-then-bf16)."""
    i = torch.arange(inter, dtype=torch.int32)[None, :] + 977 * torch.arange(rows, dtype=torch.int32)[:, None]
    up_bits = 0x3000 + i % 9728
    gate_bits = GATE32_BITS + i % 9728
    gate32 = from_bits(torch.full((rows, inter), GATE32_BITS, dtype=torch.int32))
    one = torch.ones(rows, inter, dtype=BF)
    return {"up_in": torch.cat([gate32, from_bits(up_bits)], dim=1), "up_want": from_bits(up_bits + 0x280),
            "gate_in": torch.cat([from_bits(gate_bits), one], dim=1), "gate_want": from_bits(gate_bits)}


# ----------------------------------------------------------------------------------------------------------------------
# embedding gather
# ----------------------------------------------------------------------------------------------------------------------
EMBED_VOCAB = 11
EMBED_HIDDEN = tuple(h for h in HIDDEN_EDGES if h <= 2560)
EMBED_TOKENS = (1, 77)


def embed_case(hidden: int, n_tokens: int):
    """(table [11, hidden] of distinct bit patterns, ids int32 [n_tokens], the rows the kernel must copy).  The ids hold
    0, vocab - 1, repeats, a negative id (clamped to row 0) and ids >= vocab (clamped to the last row)."""
    idx = torch.arange(EMBED_VOCAB * hidden, dtype=torch.int32)
    table = from_bits(idx + 0x0100).view(EMBED_VOCAB, hidden)          # 28 160 patterns at most: no two equal
    special = [-3, 0, EMBED_VOCAB - 1, EMBED_VOCAB, 5, 5, -(2 ** 31), 2 ** 31 - 1, 0, EMBED_VOCAB + 100]
    if n_tokens == 1:
        return table, [torch.tensor([i], dtype=torch.int32) for i in (-3, EMBED_VOCAB, 0, EMBED_VOCAB - 1, 4)]
    g = _gen("embed", hidden)
    ids = torch.cat([torch.tensor(special, dtype=torch.int32),
                     torch.randint(0, EMBED_VOCAB, (n_tokens - len(special),), generator=g, dtype=torch.int32)])
    return table, [ids]


def embed_rows(ids: torch.Tensor) -> torch.Tensor:
    return ids.long().clamp(0, EMBED_VOCAB - 1)


# ----------------------------------------------------------------------------------------------------------------------
# pooling
# ----------------------------------------------------------------------------------------------------------------------
POOL_HIDDEN = (8, 250, 2560, 8192)
POOL_CU = (0, 1, 1, 3, 11, 11)               # lengths 1, 0 (empty), 2, 8, 0 (empty, last): means over 1, 2, 8 are exact
POOL_ROWS = (13, 0, 5, 5, 13, 2)             # repeats, 0 and the last row


def pool_out_dims(hidden: int) -> Tuple[int, ...]:
    return tuple(sorted({1, min(64, hidden), hidden}))


def pool_spans(cu: Sequence[int] = POOL_CU) -> List[Tuple[int, int]]:
    return list(zip(cu[:-1], cu[1:]))


def pool_probe(hidden: int, with_delta: bool) -> Dict[str, torch.Tensor]:
    """Mode 0: 14 tokens, token t all +-C with sign signature t (C alternating); with_delta: hs = +-C/4, delta = +-3C/4.
    `normed` [14, hidden] fp64 is what the final norm must make of token t: +-w exactly."""
    sg = signs(hidden, range(N_SIGNS))
    c = torch.tensor(PROBE_C, dtype=F64)[torch.arange(N_SIGNS) % 2][:, None]
    w = pattern_weights(hidden)
    p = {"w": w, "normed": sg * w.double(), "sign": sg}
    if with_delta:
        p["hs"], p["delta"] = (sg * c / 4).float().to(BF), (sg * 3 * c / 4).float().to(BF)
    else:
        p["hs"] = (sg * c).float().to(BF)
    return p


def pool_want(row: torch.Tensor, out_dim: int) -> torch.Tensor:
    """[B, out_dim] fp64 from pooled rows [B, hidden] fp64 (zero rows stay zero)."""
    r = row[:, :out_dim]
    return r / r.norm(dim=1, keepdim=True).clamp_min(1e-12)


def pool_mean_tokens(hidden: int) -> torch.Tensor:
    """Mode 1: 14 integer-valued tokens in -8..8; over 1, 2 and 8 tokens the mean is exact in fp32."""
    return torch.randint(-8, 9, (N_SIGNS, hidden), generator=_gen("pool-mean", hidden)).to(BF)


def pool_chain_case(hidden: int):
    """(hs [14, hidden], delta, w): random rows for the chain check of the pooled row (rstd_robust, as RMSNorm's)."""
    hs, w, delta = _robust_rows("pool-chain", N_SIGNS, hidden, 1.0, True)
    return hs, delta, w


# ----------------------------------------------------------------------------------------------------------------------
# the two heads: integer setup
# ----------------------------------------------------------------------------------------------------------------------
LM_HIDDEN = (64, 192, 256, 320, 2624)        # the tail loop alone (64, 192), the main loop alone (256), both (320, 2624)
LM_ROWS = (1, 8)
LM_VOCAB = (1, 15, 16, 17, 255, 256, 257, 300)
RERANK_HIDDEN = (64, 250, 2560, 8192)
RERANK_ROWS = (7, 0, 3, 3, 7, 1)             # repeats, 0 and the last row
RERANK_KINDS = ("random", "equal", "plus200", "minus200")
INT_W = (-2.0, -1.0, 1.0, 2.0)


def int_rows(n_rows: int, hidden: int, with_delta: bool, key: str) -> Dict[str, torch.Tensor]:
    """n_rows <= 14 rows of +-C (row r: sign signature r, the last row all positive) under w in {+-1, +-2}: the normed
    rows are exactly the integers sign * w.  with_delta: hs = +-C/4, delta = +-3C/4."""
    pats = list(range(n_rows - 1)) + [N_SIGNS - 1]
    sg = signs(hidden, pats)
    c = torch.tensor(PROBE_C, dtype=F64)[torch.arange(n_rows) % 2][:, None]
    w = torch.tensor(INT_W)[torch.randint(0, 4, (hidden,), generator=_gen("int-w", hidden, key))].to(BF)
    p = {"w": w, "normed": (sg * w.double()).long(), "key": (hidden, key)}
    if with_delta:
        p["hs"], p["delta"] = (sg * c / 4).float().to(BF), (sg * 3 * c / 4).float().to(BF)
    else:
        p["hs"], p["delta"] = (sg * c).float().to(BF), None
    return p


def lm_integer(p: Dict, vocab: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lm [vocab, hidden] of integers in -3..3, the exact logits [n, vocab] int64: |logit| <= 6 hidden < 2^24)."""
    lm = torch.randint(-3, 4, (vocab, p["w"].numel()), generator=_gen("lm", vocab, p["key"]))
    return lm.to(BF), p["normed"] @ lm.long().t()


def lm_one_hot_columns(vocab: int, hidden: int) -> torch.Tensor:
    """k(v) = (7 v + 3) mod hidden: 7 is coprime to every hidden here, so vocab >= hidden walks all of 0..hidden - 1."""
    assert math.gcd(7, hidden) == 1
    return (7 * torch.arange(vocab) + 3) % hidden


def lm_one_hot(hidden: int, n_rows: int, vocab: int):
    """(hs, w of distinct patterns, lm with lm[v] = e_k(v), want [n, vocab] fp32 = float(+-w[k(v)]))."""
    pats = list(range(n_rows - 1)) + [N_SIGNS - 1]
    sg = signs(hidden, pats)
    c = torch.tensor(PROBE_C, dtype=F64)[torch.arange(n_rows) % 2][:, None]
    w = pattern_weights(hidden)
    cols = lm_one_hot_columns(vocab, hidden)
    lm = torch.zeros(vocab, hidden, dtype=BF)
    lm[torch.arange(vocab), cols] = 1.0
    return (sg * c).float().to(BF), w, lm, (sg * w.double())[:, cols].float()


# -- argmax: planted logits --------------------------------------------------------------------------------------------
ARGMAX_HIDDEN = 64
HADAMARD = torch.tensor([[(-1) ** bin(r & j).count("1") for j in range(8)] for r in range(8)], dtype=F64)


def planted(p_logits: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(hs [8, 64], w = 1, lm [V, 64]) whose exact logits are p_logits [8, V] (integer multiples of 8, small): row r of
    hs is +-C with the signs of row r of the 8 x 8 Hadamard matrix H over columns 0..7 (the other columns positive, lm
    zero there), lm[v][j] = sum_r P[r][v] H[r][j] / 8, and H H^T = 8 I."""
    assert p_logits.shape[0] == 8 and bool((p_logits % 8 == 0).all())
    sg = torch.ones(8, ARGMAX_HIDDEN, dtype=F64)
    sg[:, :8] = HADAMARD
    lm = torch.zeros(p_logits.shape[1], ARGMAX_HIDDEN, dtype=F64)
    lm[:, :8] = p_logits.double().t() @ HADAMARD / 8
    assert float(lm.abs().max()) <= 256 and bool((lm == lm.round()).all())
    c = torch.tensor(PROBE_C, dtype=F64)[torch.arange(8) % 2][:, None]
    return (sg * c).float().to(BF), torch.ones(ARGMAX_HIDDEN, dtype=BF), lm.float().to(BF)


def argmax_cases() -> Iterator[Dict]:
    """name, hs, w, lm, banned (list) -- the reference logits and tokens come from head_ref and argmax_ref; the host file
    asserts that every situation the names promise is really in the reference."""
    def base(name, vocab):
        g = _gen("argmax", name, vocab)
        return 8 * torch.randint(-8, 9, (8, vocab), generator=g)

    p = base("nan-row", 15)
    hs, w, lm = planted(p)
    hs[3] = NAN
    yield {"name": "all-NaN row", "hs": hs, "w": w, "lm": lm, "banned": []}

    hs, w, lm = planted(base("banned", 15))
    lm[2], lm[5] = NAN, NAN
    yield {"name": "every finite id banned", "hs": hs, "w": w, "lm": lm, "banned": [i for i in range(15) if i not in (2, 5)]}

    hs, w, lm = planted(base("minus-inf", 17))
    lm[:, 8] = -math.inf                      # column 8: every row of hs positive, w = 1
    lm[11, 8] = 0.0
    yield {"name": "-inf but one", "hs": hs, "w": w, "lm": lm, "banned": []}

    for vocab in (1, 16, 300):
        p = base("ends", vocab).clamp(-56, 56)
        p[0::2, 0] = 64                       # even rows: the maximum at id 0 ...
        p[1::2, vocab - 1] = 64               # ... odd rows at the last id (vocab 1: the same id)
        hs, w, lm = planted(p)
        yield {"name": f"maximum at the ends, vocab {vocab}", "hs": hs, "w": w, "lm": lm, "banned": []}

    for vocab in (1023, 1024, 1025):          # one id per thread, then a second trip
        last = vocab - 1
        pairs = [(0, last), (1, last), (1022, last), (5, 700), (last, last), (0, 1), (700, 1000), (3, last)]
        p = base("ties", vocab).clamp(-56, 56)
        for r, (a, b) in enumerate(pairs):
            p[r, a] = p[r, b] = 72
        for banned in ([], [5, 0]):
            hs, w, lm = planted(p)
            yield {"name": f"ties, vocab {vocab}, banned {banned}", "hs": hs, "w": w, "lm": lm, "banned": banned,
                   "pairs": pairs}


# -- rerank ------------------------------------------------------------------------------------------------------------
def rerank_lm(p: Dict, kind: str) -> torch.Tensor:
    """lm_rows [2, hidden] of small integers.  "random": -3..3.  "equal": yes == no.  "plus200" / "minus200": against the
    all-positive row (the last), 50 columns contribute 2 each to one logit and -2 to the other: +-100 and -+100."""
    hidden = p["w"].numel()
    if kind == "random":
        return torch.randint(-3, 4, (2, hidden), generator=_gen("rerank", kind, p["key"])).to(BF)
    if kind == "equal":
        return torch.randint(-3, 4, (1, hidden), generator=_gen("rerank", kind, p["key"])).expand(2, hidden).contiguous().to(BF)
    w = p["w"].double()
    row = torch.where(torch.arange(hidden) < 50, 2.0 / w, torch.zeros(()).double())     # w * row = 2 on 50 columns
    yes = row if kind == "plus200" else -row
    return torch.stack([yes, -yes]).float().to(BF)
