"""torch-tensor wrappers over the crag_enc_* C ABI (include/crag_encoder.h).  Tensors must be
contiguous CUDA tensors; bf16 tensors are passed as raw storage.  No CPU fallback."""
from __future__ import annotations

import ctypes

import torch

from .. import _native


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _req(t: torch.Tensor, dtype, name: str) -> None:
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous CUDA tensor of dtype {dtype}")


def embed_gather(ids: torch.Tensor, table: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    _req(ids, torch.int32, "ids"); _req(table, torch.bfloat16, "table"); _req(out, torch.bfloat16, "out")
    _native.check(_native.load().crag_enc_embed_gather(_p(ids), _p(table), _p(out), ids.numel(), table.shape[1],
                                                       table.shape[0], _stream()), "crag_enc_embed_gather")
    return out


def rmsnorm(x, weight, out, eps: float, residual_in=None, residual_out=None):
    _req(x, torch.bfloat16, "x"); _req(weight, torch.bfloat16, "weight"); _req(out, torch.bfloat16, "out")
    rows, hidden = x.shape
    _native.check(_native.load().crag_enc_rmsnorm(_p(x), _p(residual_in), _p(weight), _p(out), _p(residual_out),
                                                  rows, hidden, float(eps), _stream()), "crag_enc_rmsnorm")
    return out


def qk_norm_rope(qkv, q_w, k_w, cos_sin, positions, hq: int, hkv: int, eps: float):
    _req(qkv, torch.bfloat16, "qkv"); _req(cos_sin, torch.float32, "cos_sin"); _req(positions, torch.int32, "positions")
    _native.check(_native.load().crag_enc_qk_norm_rope(_p(qkv), _p(q_w), _p(k_w), _p(cos_sin), _p(positions),
                                                       positions.numel(), hq, hkv, float(eps), _stream()),
                  "crag_enc_qk_norm_rope")
    return qkv


def v_transpose(qkv, vt, tok_of_pad, hq: int, hkv: int):
    _req(qkv, torch.bfloat16, "qkv"); _req(vt, torch.bfloat16, "vt"); _req(tok_of_pad, torch.int32, "tok_of_pad")
    _native.check(_native.load().crag_enc_v_transpose(_p(qkv), _p(vt), _p(tok_of_pad), tok_of_pad.numel(), hq, hkv,
                                                      _stream()), "crag_enc_v_transpose")
    return vt


def attention(qkv, vt, out, cu, cu_pad, blk_seq, blk_q0, hq: int, hkv: int, scale: float):
    _req(qkv, torch.bfloat16, "qkv"); _req(vt, torch.bfloat16, "vt"); _req(out, torch.bfloat16, "out")
    _native.check(_native.load().crag_enc_attention(_p(qkv), _p(vt), _p(out), _p(cu), _p(cu_pad), _p(blk_seq),
                                                    _p(blk_q0), blk_seq.numel(), vt.shape[-1], hq, hkv, float(scale),
                                                    _stream()), "crag_enc_attention")
    return out


def swiglu(gate_up, out):
    _req(gate_up, torch.bfloat16, "gate_up"); _req(out, torch.bfloat16, "out")
    rows, two_i = gate_up.shape
    _native.check(_native.load().crag_enc_swiglu(_p(gate_up), _p(out), rows, two_i // 2, _stream()), "crag_enc_swiglu")
    return out


def pool_normalize(hidden_states, final_norm_w, cu, out, out_dim: int, mode: int, eps: float, delta=None):
    _req(hidden_states, torch.bfloat16, "hidden_states"); _req(out, torch.float32, "out")
    if delta is not None:
        _req(delta, torch.bfloat16, "delta")
        if delta.shape != hidden_states.shape:
            raise ValueError("delta must have the shape of hidden_states")
    _native.check(_native.load().crag_enc_pool_normalize_add(_p(hidden_states), _p(delta), _p(final_norm_w), _p(cu),
                                                             _p(out), cu.numel() - 1, hidden_states.shape[1], out_dim,
                                                             mode, float(eps), _stream()), "crag_enc_pool_normalize")
    return out


def pool_normalize_rows(hidden_states, final_norm_w, rows, out, out_dim: int, eps: float, delta=None):
    """Last-token pooling + final RMSNorm + slice + L2 normalise of the rows `rows` (int64 [B], device) of hidden_states
    (+ delta): crag_enc_pool_normalize_rows -- the pooled rows are data, nothing is gathered first."""
    _req(hidden_states, torch.bfloat16, "hidden_states"); _req(out, torch.float32, "out"); _req(rows, torch.int64, "rows")
    if delta is not None:
        _req(delta, torch.bfloat16, "delta")
        if delta.shape != hidden_states.shape:
            raise ValueError("delta must have the shape of hidden_states")
    _native.check(_native.load().crag_enc_pool_normalize_rows(_p(hidden_states), _p(delta), _p(final_norm_w), _p(rows),
                                                              _p(out), rows.numel(), hidden_states.shape[1], out_dim,
                                                              float(eps), _stream()), "crag_enc_pool_normalize_rows")
    return out


def skinny_weight(weight: torch.Tensor) -> torch.Tensor:
    """[n, k] bf16 (torch Linear layout) -> the MFMA A-fragment order crag_enc_skinny_gemm streams
    ([n/16][k/32][lane = 16 (kk/8) + row][8]); n % 16 == 0, k % 32 == 0."""
    n, k = weight.shape
    return weight.view(n // 16, 16, k // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()


def skinny_gate_up_weight(gate_up: torch.Tensor) -> torch.Tensor:
    """The fused [2I, k] gate|up weight with rows interleaved per 8 features (tile t = gate rows 8t..8t+7, then up rows
    8t..8t+7), in fragment order: the operand of skinny_gemm(..., swiglu=True)."""
    two_i, k = gate_up.shape
    inter = two_i // 2
    g = gate_up[:inter].view(inter // 8, 8, k)
    u = gate_up[inter:].view(inter // 8, 8, k)
    return skinny_weight(torch.cat([g, u], dim=1).reshape(two_i, k))


def skinny_gemm(x: torch.Tensor, wsw: torch.Tensor, out: torch.Tensor, m_rows: int, n: int, swiglu: bool = False):
    """out[m_rows, n (or n/2)] = x[m_pad, k] @ W^T for m_pad = 16 or 32 token rows (crag_enc_skinny_gemm)."""
    _req(x, torch.bfloat16, "x"); _req(wsw, torch.bfloat16, "wsw"); _req(out, torch.bfloat16, "out")
    m_pad, k = x.shape
    _native.check(_native.load().crag_enc_skinny_gemm(_p(x), _p(wsw), _p(out), int(m_rows), int(m_pad), int(n), int(k),
                                                      1 if swiglu else 0, _stream()), "crag_enc_skinny_gemm")
    return out


def qk_rope_vt(qkv, q_w, k_w, cos_sin, positions, hq: int, hkv: int, eps: float, vt, tok_of_pad):
    """qk_norm_rope (in place on q|k) and v_transpose (v -> vt) in one launch."""
    _req(qkv, torch.bfloat16, "qkv"); _req(cos_sin, torch.float32, "cos_sin"); _req(positions, torch.int32, "positions")
    _req(vt, torch.bfloat16, "vt"); _req(tok_of_pad, torch.int32, "tok_of_pad")
    _native.check(_native.load().crag_enc_qk_rope_vt(_p(qkv), _p(q_w), _p(k_w), _p(cos_sin), _p(positions),
                                                     positions.numel(), hq, hkv, float(eps), _p(vt), _p(tok_of_pad),
                                                     tok_of_pad.numel(), _stream()), "crag_enc_qk_rope_vt")
    return qkv


# -- the layer at 16 / 32 token rows as five launches (csrc/crag_encoder_small.hip) -------------------------------
def small_weight(weight: torch.Tensor, rows: int) -> torch.Tensor:
    """[n, k] bf16 (torch Linear layout) -> the tile order crag_enc_small_gemm streams:
    [n / rows][k / 32][4][rows][8]; n % rows == 0, k % 32 == 0.  rows = 16 is skinny_weight's order."""
    n, k = weight.shape
    if n % rows or k % 32:
        raise ValueError(f"weight [{n}, {k}] does not split into {rows}-row tiles of 32-element k-steps")
    return weight.view(n // rows, rows, k // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()


def small_gemm(x: torch.Tensor, wsw: torch.Tensor, out: torch.Tensor, m_rows: int, n: int, rows: int, *,
               swiglu: bool = False, delta=None, norm_w=None, res_out=None, eps: float = 1e-6):
    """out[m_rows, n (or n/2)] = X @ W^T for 16 or 32 rows; with norm_w: X = RMSNorm(x + delta) * norm_w computed in
    the kernel's prologue, res_out <- x + delta (crag_enc_small_gemm)."""
    _req(x, torch.bfloat16, "x"); _req(wsw, torch.bfloat16, "wsw"); _req(out, torch.bfloat16, "out")
    for name, t in (("delta", delta), ("norm_w", norm_w), ("res_out", res_out)):
        if t is not None:
            _req(t, torch.bfloat16, name)
    m_pad, k = x.shape
    _native.check(_native.load().crag_enc_small_gemm(_p(x), _p(delta), _p(norm_w), _p(res_out), _p(wsw), _p(out),
                                                     int(m_rows), int(m_pad), int(n), int(k), int(rows),
                                                     1 if swiglu else 0, float(eps), _stream()), "crag_enc_small_gemm")
    return out


def small_attention(qkv, q_w, k_w, cos_sin, positions, out, hq: int, hkv: int, eps: float, scale: float,
                    by_token: bool = False):
    """q/k-norm + RoPE + causal attention of <= 32 packed token rows (crag_enc_small_attention); qkv is not modified.
    by_token: cos_sin holds the table rows of the tokens' positions, [T, 64, 2]."""
    _req(qkv, torch.bfloat16, "qkv"); _req(cos_sin, torch.float32, "cos_sin"); _req(positions, torch.int32, "positions")
    _req(out, torch.bfloat16, "out"); _req(q_w, torch.bfloat16, "q_w"); _req(k_w, torch.bfloat16, "k_w")
    _native.check(_native.load().crag_enc_small_attention(_p(qkv), _p(q_w), _p(k_w), _p(cos_sin), 1 if by_token else 0,
                                                          _p(positions), _p(out),
                                                          positions.numel(), hq, hkv, float(eps), float(scale),
                                                          _stream()), "crag_enc_small_attention")
    return out


def small_attention_seqs(qkv, q_w, k_w, cos_sin, positions, cu, n_seqs: int, max_len: int, out, hq: int, hkv: int,
                         eps: float, scale: float, by_token: bool = False):
    """q/k-norm + RoPE + causal attention of a packed batch of short sequences (every one <= max_len <= 32 tokens) in
    one launch, one workgroup per (q head, sequence) (crag_enc_small_attention_seqs); qkv is not modified."""
    _req(qkv, torch.bfloat16, "qkv"); _req(cos_sin, torch.float32, "cos_sin"); _req(positions, torch.int32, "positions")
    _req(out, torch.bfloat16, "out"); _req(q_w, torch.bfloat16, "q_w"); _req(k_w, torch.bfloat16, "k_w")
    _req(cu, torch.int32, "cu")
    _native.check(_native.load().crag_enc_small_attention_seqs(_p(qkv), _p(q_w), _p(k_w), _p(cos_sin),
                                                               1 if by_token else 0, _p(positions), _p(cu), int(n_seqs),
                                                               int(max_len), _p(out), hq, hkv, float(eps), float(scale),
                                                               _stream()), "crag_enc_small_attention_seqs")
    return out


def small_attention_seqs_parts(parts, splitk: int, m_pad: int, q_w, k_w, cos_sin, positions, cu, n_seqs: int, max_len: int,
                               out, hq: int, hkv: int, eps: float, scale: float, by_token: bool = False):
    """small_attention_seqs over the qkv projection's split-K partial tiles (wide_gemm_rows): the head vectors are summed
    over the splits and rounded to bf16 while they are loaded (crag_enc_small_attention_seqs_parts)."""
    _req(parts, torch.float32, "parts"); _req(cos_sin, torch.float32, "cos_sin"); _req(positions, torch.int32, "positions")
    _req(out, torch.bfloat16, "out"); _req(q_w, torch.bfloat16, "q_w"); _req(k_w, torch.bfloat16, "k_w")
    _req(cu, torch.int32, "cu")
    _native.check(_native.load().crag_enc_small_attention_seqs_parts(_p(parts), int(splitk), int(m_pad), _p(q_w), _p(k_w),
                                                                     _p(cos_sin), 1 if by_token else 0, _p(positions),
                                                                     _p(cu), int(n_seqs), int(max_len), _p(out), hq, hkv,
                                                                     float(eps), float(scale), _stream()),
                  "crag_enc_small_attention_seqs_parts")
    return out


# -- the linear layers at 64 / 128 token rows (csrc/crag_encoder_wide.hip) ------------------------------------------
def wide_weight(weight: torch.Tensor) -> torch.Tensor:
    """[n, k] bf16 (torch Linear layout) -> the A-fragment order of v_mfma_f32_32x32x16_bf16 that crag_enc_wide_gemm
    streams: [n/32][k/16][lane = 32 (kk/8) + row][8]; n % 128 == 0, k % 128 == 0."""
    n, k = weight.shape
    if n % 128 or k % 128:
        raise ValueError(f"weight [{n}, {k}] does not split into 128-row tiles of 128-element chunks")
    return weight.view(n // 32, 32, k // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous()


def wide_gate_up_weight(gate_up: torch.Tensor) -> torch.Tensor:
    """The fused [2I, k] gate|up weight with every 32 rows = 16 gate rows then the 16 up rows of the same features, in
    fragment order: the operand of wide_gemm(..., swiglu=True)."""
    two_i, k = gate_up.shape
    inter = two_i // 2
    g = gate_up[:inter].view(inter // 16, 16, k)
    u = gate_up[inter:].view(inter // 16, 16, k)
    return wide_weight(torch.cat([g, u], dim=1).reshape(two_i, k))


_wide_scratch: dict = {}


def wide_gemm(x: torch.Tensor, ww: torch.Tensor, out: torch.Tensor, m_rows: int, n: int, splitk: int,
              swiglu: bool = False, scratch: "torch.Tensor | None" = None):
    """out[m_rows, n (or n/2)] = x[m_pad, k] @ W^T for m_pad = 32, 64, 96 or 128 token rows: crag_enc_wide_gemm (split-K partial
    tiles, fp32) + crag_enc_wide_reduce (sum of the splits, one rounding to bf16, optional SwiGLU).  scratch: fp32
    buffer of >= splitk * n * m_pad elements (one per device is kept otherwise: calls on one stream reuse it in order)."""
    _req(x, torch.bfloat16, "x"); _req(ww, torch.bfloat16, "ww"); _req(out, torch.bfloat16, "out")
    m_pad, k = x.shape
    if int(splitk) == 1:   # one launch: the GEMM kernel rounds and writes the output itself
        _native.check(_native.load().crag_enc_wide_gemm_direct(_p(x), _p(ww), _p(out), int(m_rows), int(m_pad), int(n), int(k),
                                                               1 if swiglu else 0, _stream()), "crag_enc_wide_gemm_direct")
        return out
    need = int(splitk) * int(n) * int(m_pad)
    if scratch is None:
        scratch = _wide_scratch.get(x.device)
        if scratch is None or scratch.numel() < need:
            scratch = _wide_scratch[x.device] = torch.empty(max(need, 4 * 19456 * 128), dtype=torch.float32, device=x.device)
    elif scratch.dtype != torch.float32 or scratch.numel() < need:
        raise ValueError("scratch must be a float32 tensor of at least splitk * n * m_pad elements")
    lib = _native.load()
    _native.check(lib.crag_enc_wide_gemm(_p(x), _p(ww), _p(scratch), int(m_pad), int(n), int(k), int(splitk), _stream()),
                  "crag_enc_wide_gemm")
    _native.check(lib.crag_enc_wide_reduce(_p(scratch), _p(out), int(m_rows), int(m_pad), int(n), int(splitk),
                                           1 if swiglu else 0, _stream()), "crag_enc_wide_reduce")
    return out


def wide_gemm_rows(x: torch.Tensor, ww: torch.Tensor, n: int, splitk: int, scratch: "torch.Tensor | None" = None):
    """The split-K half of wide_gemm alone, its fp32 partial tiles TOKEN-MAJOR ([splitk, m_pad, n]) for
    rmsnorm_partials to consume (crag_enc_wide_gemm_rows).  Returns the scratch tensor that holds them: the per-device
    buffer unless one is passed -- valid until the next split-K wide_gemm / wide_gemm_rows on that device."""
    _req(x, torch.bfloat16, "x"); _req(ww, torch.bfloat16, "ww")
    m_pad, k = x.shape
    need = int(splitk) * int(n) * int(m_pad)
    if scratch is None:
        scratch = _wide_scratch.get(x.device)
        if scratch is None or scratch.numel() < need:
            scratch = _wide_scratch[x.device] = torch.empty(max(need, 4 * 19456 * 128), dtype=torch.float32, device=x.device)
    elif scratch.dtype != torch.float32 or scratch.numel() < need:
        raise ValueError("scratch must be a float32 tensor of at least splitk * n * m_pad elements")
    _native.check(_native.load().crag_enc_wide_gemm_rows(_p(x), _p(ww), _p(scratch), int(m_pad), int(n), int(k), int(splitk),
                                                         _stream()), "crag_enc_wide_gemm_rows")
    return scratch


def rmsnorm_partials(partial_rows: torch.Tensor, splitk: int, m_pad: int, weight: torch.Tensor, out: torch.Tensor,
                     eps: float, residual_in: torch.Tensor, residual_out: "torch.Tensor | None"):
    """out = RMSNorm(residual_in + bf16(sum of the splitk token-major partial tiles)) * weight; residual_out <- the sum
    (crag_enc_rmsnorm_partials: wide_reduce + rmsnorm in one launch, the same roundings)."""
    _req(partial_rows, torch.float32, "partial_rows"); _req(weight, torch.bfloat16, "weight"); _req(out, torch.bfloat16, "out")
    _req(residual_in, torch.bfloat16, "residual_in")
    rows, hidden = out.shape
    _native.check(_native.load().crag_enc_rmsnorm_partials(_p(partial_rows), int(splitk), int(m_pad), _p(residual_in), _p(weight),
                                                           _p(out), _p(residual_out), int(rows), int(hidden), float(eps),
                                                           _stream()), "crag_enc_rmsnorm_partials")
    return out


# -- the reranker's forward (csrc/crag_attention.hip, csrc/crag_rerank.hip) ------------------------------------------
def attention_prefixed(qkv, vt, out, cu, cu_pad, blk_seq, blk_q0, parent, hq: int, hkv: int, scale: float):
    """attention() where a sequence may name a parent segment (parent int32 [B], -1 = root): a child's queries see all
    of the parent's keys, then their own causally (crag_enc_attention_prefixed)."""
    _req(qkv, torch.bfloat16, "qkv"); _req(vt, torch.bfloat16, "vt"); _req(out, torch.bfloat16, "out")
    _req(parent, torch.int32, "parent")
    if parent.numel() != cu.numel() - 1:
        raise ValueError("parent needs one entry per sequence")
    _native.check(_native.load().crag_enc_attention_prefixed(_p(qkv), _p(vt), _p(out), _p(cu), _p(cu_pad), _p(blk_seq),
                                                             _p(blk_q0), _p(parent), blk_seq.numel(), vt.shape[-1], hq,
                                                             hkv, float(scale), _stream()),
                  "crag_enc_attention_prefixed")
    return out


def rerank_head(hidden_states, final_norm_w, rows, lm_rows, out, eps: float, delta=None):
    """Per pair b: final RMSNorm of hidden_states[rows[b]] (+ delta), fp32 dots with lm_rows[0] ("yes") and lm_rows[1]
    ("no"); out [n, 3] fp32 = (logit_yes, logit_no, score) (crag_enc_rerank_head)."""
    _req(hidden_states, torch.bfloat16, "hidden_states"); _req(final_norm_w, torch.bfloat16, "final_norm_w")
    _req(rows, torch.int64, "rows"); _req(lm_rows, torch.bfloat16, "lm_rows"); _req(out, torch.float32, "out")
    hidden = hidden_states.shape[1]
    if lm_rows.shape != (2, hidden) or out.shape != (rows.numel(), 3):
        raise ValueError("lm_rows must be [2, hidden] and out [n, 3]")
    if delta is not None:
        _req(delta, torch.bfloat16, "delta")
        if delta.shape != hidden_states.shape:
            raise ValueError("delta must have the shape of hidden_states")
    _native.check(_native.load().crag_enc_rerank_head(_p(hidden_states), _p(delta), _p(final_norm_w), _p(rows),
                                                      _p(lm_rows), _p(out), rows.numel(), hidden, float(eps), _stream()),
                  "crag_enc_rerank_head")
    return out


# -- autoregressive decoding (csrc/crag_decode.hip) ------------------------------------------------------------------
def decode_workspace(n_seqs: int, hq: int, max_len: int, device) -> torch.Tensor:
    """Device scratch of decode_attention for up to n_seqs sequences over caches of max_len rows (uint8)."""
    need = int(_native.load().crag_enc_decode_workspace_bytes(int(n_seqs), int(hq), int(max_len)))
    if need <= 0:
        raise ValueError(f"no decode workspace for n_seqs={n_seqs}, hq={hq}, max_len={max_len}")
    return torch.empty(need, dtype=torch.uint8, device=device)


def decode_attention(qkv_new, q_w, k_w, cos_sin, k_cache, v_cache, slots, cache_len, out, hq: int, hkv: int, eps: float,
                     scale: float, workspace):
    """One new token per sequence against ONE layer's cache (crag_enc_decode_attention).  qkv_new [n, (hq + 2 hkv) * 128]
    raw projections; k_cache / v_cache [n_slots, hkv, max_len, 128] bf16; slots / cache_len: HOST ints per sequence (the
    slot, and how many tokens it holds = the new token's position).  The new key and value are appended at position
    cache_len of the slot; out [n, hq * 128]."""
    _req(qkv_new, torch.bfloat16, "qkv_new"); _req(cos_sin, torch.float32, "cos_sin"); _req(out, torch.bfloat16, "out")
    _req(k_cache, torch.bfloat16, "k_cache"); _req(v_cache, torch.bfloat16, "v_cache")
    _req(q_w, torch.bfloat16, "q_w"); _req(k_w, torch.bfloat16, "k_w"); _req(workspace, torch.uint8, "workspace")
    n = len(slots)
    if len(cache_len) != n:
        raise ValueError("slots and cache_len need one entry per sequence")
    n_slots, kv_heads, max_len, dim = k_cache.shape
    if v_cache.shape != k_cache.shape or kv_heads != hkv or dim != 128:
        raise ValueError("k_cache and v_cache must both be [n_slots, hkv, max_len, 128]")
    if n <= _native.CRAG_DECODE_MAX_SEQS and (qkv_new.shape[0] < n or out.shape[0] < n
                                              or qkv_new.shape[1] != (hq + 2 * hkv) * 128 or out.shape[1] != hq * 128):
        raise ValueError("qkv_new must be [n, (hq + 2 hkv) * 128] and out [n, hq * 128]")
    h_slots = (ctypes.c_int32 * max(n, 1))(*[int(s) for s in slots])
    h_lens = (ctypes.c_int32 * max(n, 1))(*[int(x) for x in cache_len])
    _native.check(_native.load().crag_enc_decode_attention(
        _p(qkv_new), _p(q_w), _p(k_w), _p(cos_sin), int(cos_sin.shape[0]), _p(k_cache), _p(v_cache), int(n_slots),
        int(max_len), h_slots, h_lens, n, int(hq), int(hkv), float(eps), float(scale), _p(workspace),
        int(workspace.numel()), _p(out), _stream()), "crag_enc_decode_attention")
    return out


def decode_attention_shared(qkv_new, q_w, k_w, cos_sin, k_cache, v_cache, slots, cache_len, parents, shared_len, out,
                            hq: int, hkv: int, eps: float, scale: float, workspace):
    """decode_attention over forked sequences (crag_enc_decode_attention_shared).  parents / shared_len: HOST ints per
    sequence -- logical row j of sequence b is row j of slot parents[b] when j < shared_len[b] and of slots[b] otherwise;
    parents[b] == slots[b] or shared_len[b] == 0: not forked.  The new key and value go to row cache_len of slots[b].
    The bits of out and of the appended rows are decode_attention's on private copies of the logical rows; two
    sequences of one parent read every wholly shared split with one load.  The workspace is decode_workspace's."""
    _req(qkv_new, torch.bfloat16, "qkv_new"); _req(cos_sin, torch.float32, "cos_sin"); _req(out, torch.bfloat16, "out")
    _req(k_cache, torch.bfloat16, "k_cache"); _req(v_cache, torch.bfloat16, "v_cache")
    _req(q_w, torch.bfloat16, "q_w"); _req(k_w, torch.bfloat16, "k_w"); _req(workspace, torch.uint8, "workspace")
    n = len(slots)
    if len(cache_len) != n or len(parents) != n or len(shared_len) != n:
        raise ValueError("slots, cache_len, parents and shared_len need one entry per sequence")
    n_slots, kv_heads, max_len, dim = k_cache.shape
    if v_cache.shape != k_cache.shape or kv_heads != hkv or dim != 128:
        raise ValueError("k_cache and v_cache must both be [n_slots, hkv, max_len, 128]")
    if n <= _native.CRAG_DECODE_MAX_SEQS and (qkv_new.shape[0] < n or out.shape[0] < n
                                              or qkv_new.shape[1] != (hq + 2 * hkv) * 128 or out.shape[1] != hq * 128):
        raise ValueError("qkv_new must be [n, (hq + 2 hkv) * 128] and out [n, hq * 128]")
    h_slots, h_lens, h_parents, h_shared = ((ctypes.c_int32 * max(n, 1))(*[int(x) for x in xs])
                                            for xs in (slots, cache_len, parents, shared_len))
    _native.check(_native.load().crag_enc_decode_attention_shared(
        _p(qkv_new), _p(q_w), _p(k_w), _p(cos_sin), int(cos_sin.shape[0]), _p(k_cache), _p(v_cache), int(n_slots),
        int(max_len), h_slots, h_lens, h_parents, h_shared, n, int(hq), int(hkv), float(eps), float(scale), _p(workspace),
        int(workspace.numel()), _p(out), _stream()), "crag_enc_decode_attention_shared")
    return out


def decode_attention_rows(qkv_new, q_w, k_w, cos_sin, k_cache, v_cache, slots, cache_len, new_len, out, hq: int, hkv: int,
                          eps: float, scale: float, workspace, parents=None, shared_len=None):
    """decode_attention_shared with new_len[b] >= 1 new rows per sequence (crag_enc_decode_attention_rows): the R =
    sum(new_len) <= 8 rows of qkv_new / out lie back to back in call order, row i of sequence b is appended at row
    cache_len[b] + i of slots[b] and attends the logical rows up to itself.  parents / shared_len: None together (nobody
    is forked), or as in decode_attention_shared.  The bits of out and of the appended rows are those of new_len[b]
    successive decode_attention calls.  The workspace is decode_workspace(R, ...)'s, indexed by row."""
    _req(qkv_new, torch.bfloat16, "qkv_new"); _req(cos_sin, torch.float32, "cos_sin"); _req(out, torch.bfloat16, "out")
    _req(k_cache, torch.bfloat16, "k_cache"); _req(v_cache, torch.bfloat16, "v_cache")
    _req(q_w, torch.bfloat16, "q_w"); _req(k_w, torch.bfloat16, "k_w"); _req(workspace, torch.uint8, "workspace")
    n = len(slots)
    if (parents is None) != (shared_len is None):
        raise ValueError("parents and shared_len come together")
    lists = [slots, cache_len, new_len] + ([] if parents is None else [parents, shared_len])
    if any(len(xs) != n for xs in lists):
        raise ValueError("slots, cache_len, new_len, parents and shared_len need one entry per sequence")
    n_slots, kv_heads, max_len, dim = k_cache.shape
    if v_cache.shape != k_cache.shape or kv_heads != hkv or dim != 128:
        raise ValueError("k_cache and v_cache must both be [n_slots, hkv, max_len, 128]")
    rows = sum(max(int(m), 0) for m in new_len)
    if rows <= _native.CRAG_DECODE_MAX_ROWS and (qkv_new.shape[0] < rows or out.shape[0] < rows
                                                 or qkv_new.shape[1] != (hq + 2 * hkv) * 128 or out.shape[1] != hq * 128):
        raise ValueError("qkv_new must be [R, (hq + 2 hkv) * 128] and out [R, hq * 128]")
    h = [(ctypes.c_int32 * max(n, 1))(*[int(x) for x in xs]) for xs in lists] + [None, None]
    _native.check(_native.load().crag_enc_decode_attention_rows(
        _p(qkv_new), _p(q_w), _p(k_w), _p(cos_sin), int(cos_sin.shape[0]), _p(k_cache), _p(v_cache), int(n_slots),
        int(max_len), h[0], h[1], h[2], h[3], h[4], n, int(hq), int(hkv), float(eps), float(scale), _p(workspace),
        int(workspace.numel()), _p(out), _stream()), "crag_enc_decode_attention_rows")
    return out


def lm_head(hidden_states, final_norm_w, lm, logits, token, eps: float, delta=None, banned=None):
    """Final RMSNorm of hidden_states [n <= 8, hidden] (+ delta), fp32 logits [n, vocab] against lm [vocab, hidden] and the
    greedy token [n] int32: lowest id among the maxima, `banned` (int32 device list) left out (crag_enc_lm_head)."""
    _req(hidden_states, torch.bfloat16, "hidden_states"); _req(final_norm_w, torch.bfloat16, "final_norm_w")
    _req(lm, torch.bfloat16, "lm"); _req(logits, torch.float32, "logits"); _req(token, torch.int32, "token")
    n, hidden = hidden_states.shape
    vocab = lm.shape[0]
    if lm.shape[1] != hidden or logits.shape != (n, vocab) or token.numel() != n:
        raise ValueError("lm must be [vocab, hidden], logits [n, vocab] and token [n]")
    if delta is not None:
        _req(delta, torch.bfloat16, "delta")
        if delta.shape != hidden_states.shape:
            raise ValueError("delta must have the shape of hidden_states")
    if banned is not None:
        _req(banned, torch.int32, "banned")
    _native.check(_native.load().crag_enc_lm_head(_p(hidden_states), _p(delta), _p(final_norm_w), _p(lm), _p(logits),
                                                  _p(token), _p(banned), 0 if banned is None else banned.numel(), n,
                                                  hidden, vocab, float(eps), _stream()), "crag_enc_lm_head")
    return logits, token


# -- greedy selection under a byte automaton (csrc/crag_grammar.hip) ---------------------------------------------------
def grammar_argmax(logits, tok_offsets, tok_bytes, tok_kind, class_of, trans, accept, state, token, allowed_bits=None):
    """Per row of logits [n <= 8, vocab] fp32: token[r] (int32) = the lowest id among the maxima over the tokens the
    automaton allows in state[r] (int32, device, updated in place to the chosen token's end state), -1 when nothing is
    allowed (crag_enc_grammar_argmax).  tok_offsets [vocab + 1] int32 / tok_bytes uint8 / tok_kind [vocab] uint8: the
    token table; class_of [256] uint8, trans [n_states, n_classes] uint16 (stored as int16), accept [n_states] uint8:
    the automaton.  allowed_bits (optional) [n, ceil(vocab / 32)] int32 receives the allowed flags."""
    _req(logits, torch.float32, "logits"); _req(tok_offsets, torch.int32, "tok_offsets")
    _req(tok_bytes, torch.uint8, "tok_bytes"); _req(tok_kind, torch.uint8, "tok_kind")
    _req(class_of, torch.uint8, "class_of"); _req(trans, torch.int16, "trans"); _req(accept, torch.uint8, "accept")
    _req(state, torch.int32, "state"); _req(token, torch.int32, "token")
    if logits.dim() != 2 or trans.dim() != 2:
        raise ValueError("logits must be [n, vocab] and trans [n_states, n_classes]")
    n, vocab = logits.shape
    n_states, n_classes = trans.shape
    if tok_offsets.numel() != vocab + 1 or tok_kind.numel() != vocab or class_of.numel() != 256 \
            or accept.numel() != n_states or state.numel() != n or token.numel() != n:
        raise ValueError("tok_offsets must be [vocab + 1], tok_kind [vocab], class_of [256], accept [n_states], "
                         "state and token [n]")
    if allowed_bits is not None:
        _req(allowed_bits, torch.int32, "allowed_bits")
        if allowed_bits.shape != (n, (vocab + 31) // 32):
            raise ValueError("allowed_bits must be [n, ceil(vocab / 32)]")
    _native.check(_native.load().crag_enc_grammar_argmax(
        _p(logits), int(vocab), _p(tok_offsets), _p(tok_bytes), _p(tok_kind), _p(class_of), _p(trans), _p(accept),
        int(n_states), int(n_classes), _p(state), _p(token), _p(allowed_bits), int(n), _stream()),
        "crag_enc_grammar_argmax")
    return token, state


# -- seeded sampling (csrc/crag_sample.hip) -----------------------------------------------------------------------------
def sample(logits, params, step: int, streams, token, allowed_bits=None, kept=None, cut=None):
    """Per row of logits [n <= 8, vocab] fp32: token[r] (int32) drawn under params[r] (cadence_rag_amd.sampling
    SamplingParams; one for all rows, or one per row -- every row then carries the same seed) with the noise of
    (seed; token id, step, streams[r]) (crag_enc_sample; the rule: sampling.sample_host).  allowed_bits (optional)
    [n, ceil(vocab / 32)] int32: grammar_argmax's flags, only set ids are candidates.  kept (optional) int32 [n] /
    cut (optional) float32 [n] receive the number of ids the cuts keep and the lowest kept logit."""
    from ..sampling import SamplingParams, min_p_cut
    _req(logits, torch.float32, "logits"); _req(token, torch.int32, "token")
    if logits.dim() != 2:
        raise ValueError("logits must be [n, vocab]")
    n, vocab = logits.shape
    rows = [params] * n if isinstance(params, SamplingParams) else list(params)
    streams = [int(s) for s in streams]
    if len(rows) != n or len(streams) != n or token.numel() != n:
        raise ValueError("params, streams and token need one entry per row")
    if len({int(p.seed) for p in rows}) > 1:
        raise ValueError("one call draws with one seed: every row's params must carry the same")
    if allowed_bits is not None:
        _req(allowed_bits, torch.int32, "allowed_bits")
        if allowed_bits.shape != (n, (vocab + 31) // 32):
            raise ValueError("allowed_bits must be [n, ceil(vocab / 32)]")
    if kept is not None:
        _req(kept, torch.int32, "kept")
    if cut is not None:
        _req(cut, torch.float32, "cut")
    if (kept is not None and kept.numel() != n) or (cut is not None and cut.numel() != n):
        raise ValueError("kept and cut must be [n]")
    m = max(n, 1)
    h_t = (ctypes.c_float * m)(*[float(p.temperature) for p in rows])
    h_k = (ctypes.c_int32 * m)(*[int(p.top_k) for p in rows])
    h_p = (ctypes.c_float * m)(*[float(p.top_p) for p in rows])
    h_m = (ctypes.c_float * m)(*[float(min_p_cut(p.temperature, p.min_p)) for p in rows])
    h_s = (ctypes.c_uint32 * m)(*[s & 0xFFFFFFFF for s in streams])
    _native.check(_native.load().crag_enc_sample(
        _p(logits), int(vocab), _p(allowed_bits), h_t, h_k, h_p, h_m, h_s, int(rows[0].seed) if rows else 0,
        int(step) & 0xFFFFFFFF, _p(token), _p(kept), _p(cut), int(n), _stream()), "crag_enc_sample")
    return token


def grammar_advance(tok_offsets, tok_bytes, tok_kind, class_of, trans, state, token):
    """state[r] (int32, device, in place) becomes the state behind token[r] (int32, device) walked from it; it stays for a
    stop token, for -1 and for a token the state does not allow (crag_enc_grammar_advance).  The tables are
    grammar_argmax's."""
    _req(tok_offsets, torch.int32, "tok_offsets"); _req(tok_bytes, torch.uint8, "tok_bytes")
    _req(tok_kind, torch.uint8, "tok_kind"); _req(class_of, torch.uint8, "class_of"); _req(trans, torch.int16, "trans")
    _req(state, torch.int32, "state"); _req(token, torch.int32, "token")
    if trans.dim() != 2:
        raise ValueError("trans must be [n_states, n_classes]")
    vocab = tok_kind.numel()
    n_states, n_classes = trans.shape
    n = state.numel()
    if tok_offsets.numel() != vocab + 1 or class_of.numel() != 256 or token.numel() != n:
        raise ValueError("tok_offsets must be [vocab + 1], class_of [256], state and token [n]")
    _native.check(_native.load().crag_enc_grammar_advance(
        _p(tok_offsets), _p(tok_bytes), _p(tok_kind), int(vocab), _p(class_of), _p(trans), int(n_states), int(n_classes),
        _p(state), _p(token), int(n), _stream()), "crag_enc_grammar_advance")
    return state


# -- token log-probabilities (csrc/crag_logprobs.hip) -------------------------------------------------------------------
MAX_TOP_LOGPROBS = 16   # CRAG_LOGPROBS_MAX_TOP


def logprobs(logits, token, logprob, *, allowed_bits=None, lse_all=None, lse_allowed=None, rank=None, top_id=None,
             top_logprob=None):
    """Per row of logits [n <= 8, vocab] fp32: logprob[r] (float32) = the log-probability of token[r] (int32, device)
    under the row's own softmax (crag_enc_logprobs; the rule: cadence_rag_amd.logprobs.logprobs_host).  Optional outputs:
    lse_all / lse_allowed float32 [n] (the log-sum-exp over every id that is not NaN, and over those whose bit is set in
    allowed_bits [n, ceil(vocab / 32)] int32, grammar_argmax's flags); rank int32 [n] (1 = the most likely id); top_id
    int32 / top_logprob float32 [n, n_top], n_top <= 16, given together: the most likely ids over the whole row."""
    _req(logits, torch.float32, "logits"); _req(token, torch.int32, "token"); _req(logprob, torch.float32, "logprob")
    if logits.dim() != 2:
        raise ValueError("logits must be [n, vocab]")
    n, vocab = logits.shape
    if token.numel() != n or logprob.numel() != n:
        raise ValueError("token and logprob must be [n]")
    if allowed_bits is not None:
        _req(allowed_bits, torch.int32, "allowed_bits")
        if allowed_bits.shape != (n, (vocab + 31) // 32):
            raise ValueError("allowed_bits must be [n, ceil(vocab / 32)]")
    for name, t, dtype in (("lse_all", lse_all, torch.float32), ("lse_allowed", lse_allowed, torch.float32),
                           ("rank", rank, torch.int32)):
        if t is not None:
            _req(t, dtype, name)
            if t.numel() != n:
                raise ValueError(f"{name} must be [n]")
    if (top_id is None) != (top_logprob is None):
        raise ValueError("top_id and top_logprob are given together")
    n_top = 0
    if top_id is not None:
        _req(top_id, torch.int32, "top_id"); _req(top_logprob, torch.float32, "top_logprob")
        if top_id.dim() != 2 or top_id.shape[0] != n or top_logprob.shape != top_id.shape:
            raise ValueError("top_id and top_logprob must both be [n, n_top]")
        n_top = int(top_id.shape[1])
    _native.check(_native.load().crag_enc_logprobs(
        _p(logits), int(vocab), _p(allowed_bits), _p(token), _p(logprob), _p(lse_all), _p(lse_allowed), _p(rank),
        _p(top_id) if n_top else None, _p(top_logprob) if n_top else None, n_top, int(n), _stream()),
        "crag_enc_logprobs")
    return logprob


# -- repetition control (csrc/crag_penalty.hip) -------------------------------------------------------------------------
def adjust_workspace(n_rows: int, vocab: int, device) -> torch.Tensor:
    """Device scratch of adjust_logits for up to n_rows rows of vocab ids (uint8): a [vocab] int32 slice per row."""
    need = int(_native.load().crag_enc_adjust_workspace_bytes(int(n_rows), int(vocab)))
    if need <= 0:
        raise ValueError(f"no adjust workspace for n_rows={n_rows}, vocab={vocab}")
    return torch.empty(need, dtype=torch.uint8, device=device)


def adjust_logits(logits, out, history, history_rows, prompt_lens, total_lens, params, token, workspace, *,
                  exempt_bits=None, bias_ids=None, bias_values=None, bias_offsets=None):
    """Per row of logits [n <= 8, vocab] fp32: out[r] (fp32, may be logits itself) = the row under params[r]
    (cadence_rag_amd.penalties PenaltyParams; one for all rows, or one per row) and token[r] (int32) = the lowest id among
    its maxima (crag_enc_adjust_logits; the rule: penalties.adjust_host).  history [rows, stride] int32 is a token log on
    the device: row r reads the first total_lens[r] ids of log row history_rows[r], the first prompt_lens[r] of them its
    prompt (HOST ints).  exempt_bits (optional) [ceil(vocab / 32)] int32, shared by the rows: ids no penalty touches.
    bias_ids int32 / bias_values float32 (device) with bias_offsets (HOST ints, n + 1, rising from 0), given together: the
    rows' bias lists back to back, a row's ids strictly ascending -- params[r].logit_bias is NOT read here.  workspace:
    adjust_workspace(n, vocab)."""
    from ..penalties import PenaltyParams
    _req(logits, torch.float32, "logits"); _req(out, torch.float32, "out"); _req(history, torch.int32, "history")
    _req(token, torch.int32, "token"); _req(workspace, torch.uint8, "workspace")
    if logits.dim() != 2 or history.dim() != 2 or out.shape != logits.shape:
        raise ValueError("logits and out must be [n, vocab] and history [rows, stride]")
    n, vocab = logits.shape
    rows = [params] * n if isinstance(params, PenaltyParams) else list(params)
    lists = [[int(x) for x in xs] for xs in (history_rows, prompt_lens, total_lens)]
    if len(rows) != n or any(len(xs) != n for xs in lists) or token.numel() != n:
        raise ValueError("params, history_rows, prompt_lens, total_lens and token need one entry per row")
    if exempt_bits is not None:
        _req(exempt_bits, torch.int32, "exempt_bits")
        if exempt_bits.numel() != (vocab + 31) // 32:
            raise ValueError("exempt_bits must be [ceil(vocab / 32)]")
    given = [x is not None for x in (bias_ids, bias_values, bias_offsets)]
    if any(given) != all(given):
        raise ValueError("bias_ids, bias_values and bias_offsets are given together")
    h_off = None
    if all(given):
        _req(bias_ids, torch.int32, "bias_ids"); _req(bias_values, torch.float32, "bias_values")
        offsets = [int(x) for x in bias_offsets]
        if len(offsets) != n + 1 or bias_ids.numel() != bias_values.numel() or \
                (n <= _native.CRAG_DECODE_MAX_SEQS and max(offsets) > bias_ids.numel()):
            raise ValueError("bias_offsets needs n + 1 entries inside bias_ids, and bias_values one value per id")
        h_off = (ctypes.c_int32 * (n + 1))(*offsets)
    m = max(n, 1)
    h_row, h_prompt, h_total = ((ctypes.c_int32 * m)(*xs) for xs in lists)
    h_rp = (ctypes.c_float * m)(*[float(p.repetition_penalty) for p in rows])
    h_fr = (ctypes.c_float * m)(*[float(p.frequency_penalty) for p in rows])
    h_pr = (ctypes.c_float * m)(*[float(p.presence_penalty) for p in rows])
    h_ng = (ctypes.c_int32 * m)(*[int(p.no_repeat_ngram) for p in rows])
    _native.check(_native.load().crag_enc_adjust_logits(
        _p(logits), _p(out), int(vocab), _p(history), int(history.shape[1]), int(history.shape[0]), h_row, h_prompt,
        h_total, h_rp, h_fr, h_pr, h_ng, _p(exempt_bits), _p(bias_ids), _p(bias_values), h_off, _p(token), _p(workspace),
        int(workspace.numel()), int(n), _stream()), "crag_enc_adjust_logits")
    return out, token


# -- continuing cached sequences (csrc/crag_extend.hip) ---------------------------------------------------------------
def extend_workspace_bytes(n_seqs: int, hq: int, max_new_rows: int, max_len: int) -> int:
    """Bytes of scratch extend_attention needs at most for up to n_seqs sequences with up to max_new_rows new rows in
    all, none of them longer than max_len rows once extended."""
    need = int(_native.load().crag_enc_extend_workspace_bytes(int(n_seqs), int(hq), int(max_new_rows), int(max_len)))
    if need <= 0:
        raise ValueError(f"no extend workspace for n_seqs={n_seqs}, hq={hq}, max_new_rows={max_new_rows}, max_len={max_len}")
    return need


def extend_workspace(n_seqs: int, hq: int, max_new_rows: int, max_len: int, device) -> torch.Tensor:
    """Device scratch of extend_attention (extend_workspace_bytes of uint8)."""
    return torch.empty(extend_workspace_bytes(n_seqs, hq, max_new_rows, max_len), dtype=torch.uint8, device=device)


def extend_attention(qkv_new, q_w, k_w, cos_sin, k_cache, v_cache, slots, cache_len, new_len, out, hq: int, hkv: int,
                     eps: float, scale: float, workspace):
    """new_len[b] new tokens per sequence against ONE layer's cache (crag_enc_extend_attention).  qkv_new [T_new,
    (hq + 2 hkv) * 128] raw projections, the sequences' rows back to back; k_cache / v_cache [n_slots, hkv, max_len, 128]
    bf16; slots / cache_len / new_len: HOST ints per sequence.  The new keys and values are appended at positions
    cache_len .. cache_len + new_len - 1 of the slot; query row i sees the keys 0 .. cache_len + i; out [T_new, hq * 128]."""
    _req(qkv_new, torch.bfloat16, "qkv_new"); _req(cos_sin, torch.float32, "cos_sin"); _req(out, torch.bfloat16, "out")
    _req(k_cache, torch.bfloat16, "k_cache"); _req(v_cache, torch.bfloat16, "v_cache")
    _req(q_w, torch.bfloat16, "q_w"); _req(k_w, torch.bfloat16, "k_w"); _req(workspace, torch.uint8, "workspace")
    n = len(slots)
    if len(cache_len) != n or len(new_len) != n:
        raise ValueError("slots, cache_len and new_len need one entry per sequence")
    n_slots, kv_heads, max_len, dim = k_cache.shape
    if v_cache.shape != k_cache.shape or kv_heads != hkv or dim != 128:
        raise ValueError("k_cache and v_cache must both be [n_slots, hkv, max_len, 128]")
    t_new = sum(max(int(x), 0) for x in new_len)
    if qkv_new.shape[0] < t_new or out.shape[0] < t_new or qkv_new.shape[1] != (hq + 2 * hkv) * 128 \
            or out.shape[1] != hq * 128:
        raise ValueError("qkv_new must be [T_new, (hq + 2 hkv) * 128] and out [T_new, hq * 128]")
    h_slots = (ctypes.c_int32 * max(n, 1))(*[int(s) for s in slots])
    h_lens = (ctypes.c_int32 * max(n, 1))(*[int(x) for x in cache_len])
    h_new = (ctypes.c_int32 * max(n, 1))(*[int(x) for x in new_len])
    _native.check(_native.load().crag_enc_extend_attention(
        _p(qkv_new), _p(q_w), _p(k_w), _p(cos_sin), int(cos_sin.shape[0]), _p(k_cache), _p(v_cache), int(n_slots),
        int(max_len), h_slots, h_lens, h_new, n, int(hq), int(hkv), float(eps), float(scale), _p(workspace),
        int(workspace.numel()), _p(out), _stream()), "crag_enc_extend_attention")
    return out
