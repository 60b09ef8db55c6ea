"""Inputs and references for crag_enc_decode_attention (tests/test_decode_gpu.py): random ragged caches with NaN behind
the live rows, the fp32 formula, and one-key probes in the style of attention_probes.py -- a cache whose keys are all
zero except key j, which is the rotated query times 16, so that every other softmax weight underflows to exactly 0 and
the output must be V[j] bit for bit.

The cache is a one-layer KvCache and is filled and read through its accessors only (append_prefill, keys, values).
(rotated() takes crag_enc_qk_norm_rope as the reference; test_row_probes_gpu.py pins the appended rows without it.)"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Sequence

import torch

BF = torch.bfloat16
EPS = 1e-6
SCALE = 1.0 / math.sqrt(128)
SPLIT = 128      # CRAG_DECODE_SPLIT: keys per workgroup
TILE = 16        # keys per pass of a workgroup
LENGTHS = sorted({0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000,
                  TILE - 1, TILE, TILE + 1, SPLIT - 1, SPLIT, SPLIT + 1, 2 * SPLIT - 1, 2 * SPLIT, 2 * SPLIT + 1})


def rope_table(max_pos: int, device) -> torch.Tensor:
    inv_freq = 1.0 / (1_000_000.0 ** (torch.arange(0, 64, dtype=torch.float32) * 2.0 / 128))
    ang = torch.arange(max_pos, dtype=torch.float32)[:, None] * inv_freq[None, :]
    return torch.stack([ang.cos(), ang.sin()], dim=-1).contiguous().to(device)


@dataclass
class Case:
    hq: int
    hkv: int
    slots: List[int]
    lens: List[int]
    qkv_new: torch.Tensor     # [n, (hq + 2 hkv) * 128] bf16, device
    q_w: torch.Tensor
    k_w: torch.Tensor
    cos_sin: torch.Tensor
    cache: object             # KvCache, one layer
    workspace: torch.Tensor


def make_case(hq: int, hkv: int, lens: Sequence[int], slots: Sequence[int], *, n_slots: int = 8, max_len: int = 1024,
              seed: int = 0, device=None) -> Case:
    """Random new rows; slot slots[b] holds lens[b] random keys / values, every other cache row is NaN."""
    from cadence_rag_amd.encoder import ops
    from cadence_rag_amd.encoder.generate import KvCache
    g = torch.Generator().manual_seed(seed)
    n = len(lens)
    qkv = torch.randn(n, (hq + 2 * hkv) * 128, generator=g).to(BF).to(device)
    q_w = (1 + 0.1 * torch.randn(128, generator=g)).to(BF).to(device)
    k_w = (1 + 0.1 * torch.randn(128, generator=g)).to(BF).to(device)
    cache = KvCache(1, n_slots, hkv, max_len, device)
    cache.k.fill_(float("nan"))
    cache.v.fill_(float("nan"))
    for slot, m in zip(slots, lens):
        if m:
            cache.append_prefill(0, slot, torch.randn(m, hkv, 128, generator=g).to(BF).to(device),
                                 torch.randn(m, hkv, 128, generator=g).to(BF).to(device))
        cache.lens[slot] = m
    return Case(hq, hkv, list(slots), list(lens), qkv, q_w, k_w, rope_table(max_len, device), cache,
                ops.decode_workspace(8, hq, max_len, device))


def rotated(case: Case) -> torch.Tensor:
    """The new rows as crag_enc_qk_norm_rope leaves them at positions `lens` (q and k normed + rotated, v raw)."""
    from cadence_rag_amd.encoder import ops
    out = case.qkv_new.clone()
    pos = torch.tensor(case.lens, dtype=torch.int32, device=out.device)
    ops.qk_norm_rope(out, case.q_w, case.k_w, case.cos_sin, pos, case.hq, case.hkv, EPS)
    return out


def run(case: Case, seqs: Sequence[int] = None) -> torch.Tensor:
    """One decode call over the sequences `seqs` of the case (default all); the cache lengths grow by one."""
    from cadence_rag_amd.encoder import ops
    seqs = list(range(len(case.lens))) if seqs is None else list(seqs)
    idx = torch.tensor(seqs, device=case.qkv_new.device)
    out = torch.full((len(seqs), case.hq * 128), float("nan"), dtype=BF, device=case.qkv_new.device)
    kc, vc = case.cache.layer(0)
    slots = [case.slots[b] for b in seqs]
    ops.decode_attention(case.qkv_new.index_select(0, idx).contiguous(), case.q_w, case.k_w, case.cos_sin, kc, vc, slots,
                         [case.lens[b] for b in seqs], out, case.hq, case.hkv, EPS, SCALE, case.workspace)
    for s in slots:
        case.cache.lens[s] += 1
    torch.cuda.synchronize()
    return out


def reference(case: Case, rot: torch.Tensor) -> torch.Tensor:
    """fp32 on the CPU: softmax(q K^T / sqrt(128)) V over the slot's cached rows plus the new row.  Call BEFORE run()."""
    hq, hkv, gsz = case.hq, case.hkv, case.hq // case.hkv
    f = rot.float().cpu()
    out = torch.zeros(len(case.lens), hq, 128)
    for b, (slot, m) in enumerate(zip(case.slots, case.lens)):
        q = f[b, : hq * 128].view(hq, 128)
        k_new = f[b, hq * 128: (hq + hkv) * 128].view(1, hkv, 128)
        v_new = f[b, (hq + hkv) * 128:].view(1, hkv, 128)
        keys = torch.cat([case.cache.keys(0, slot).float().cpu(), k_new])
        vals = torch.cat([case.cache.values(0, slot).float().cpu(), v_new])
        for h in range(hq):
            w = torch.softmax((keys[:, h // gsz] @ q[h]) * SCALE, dim=0)
            out[b, h] = w @ vals[:, h // gsz]
    return out.view(len(case.lens), hq * 128)


def one_key_case(hq: int, hkv: int, js: Sequence[int], n_keys: int, *, seed: int = 0, device=None):
    """len(js) <= 8 sequences in slots 0.., each with n_keys - 1 cached keys and one new token.  Sequence b's only
    non-zero key is key js[b] = 16 x the rotated query (all query heads of a kv head share one raw query); js[b] ==
    n_keys - 1 is the new token's own key, made by the kernel from raw k = raw q under k_norm = 16 x q_norm.
    Returns (case, expected [n, hq * 128] bf16 = V[js[b]] per head)."""
    from cadence_rag_amd.encoder import ops
    from cadence_rag_amd.encoder.generate import KvCache
    g = torch.Generator().manual_seed(seed)
    n, m, gsz = len(js), n_keys - 1, hq // hkv
    q_kv = torch.randn(n, hkv, 1, 128, generator=g)
    q_raw = q_kv.expand(n, hkv, gsz, 128).reshape(n, hq * 128)
    own = torch.tensor([j == m for j in js]).view(n, 1, 1)
    k_raw = torch.where(own, q_kv[:, :, 0], torch.zeros(())).reshape(n, hkv * 128)
    v_raw = torch.randn(n, hkv * 128, generator=g)
    qkv = torch.cat([q_raw, k_raw, v_raw], dim=1).to(BF).to(device)
    q_w = (1 + 0.1 * torch.randn(128, generator=g)).to(BF)
    k_w = (q_w.float() * 16).to(BF)          # exact: a power of two
    max_len = (n_keys + 31) // 32 * 32
    cache = KvCache(1, 8, hkv, max_len, device)
    cache.k.fill_(float("nan"))
    cache.v.fill_(float("nan"))
    case = Case(hq, hkv, list(range(n)), [m] * n, qkv, q_w.to(device), k_w.to(device), rope_table(max_len, device), cache,
                ops.decode_workspace(8, hq, max_len, device))
    rot = rotated(case)
    q_rot = rot[:, : hq * 128].view(n, hkv, gsz, 128)[:, :, 0]       # [n, hkv, 128]
    vals = torch.randn(n, m, hkv, 128, generator=g).to(BF).to(device)
    want = torch.empty(n, hkv, 128, dtype=BF, device=device)
    for b, j in enumerate(js):
        keys = torch.zeros(m, hkv, 128, dtype=BF, device=device)
        if j < m:
            keys[j] = (q_rot[b].float() * 16).to(BF)
            want[b] = vals[b, j]
        else:
            want[b] = qkv[b, (hq + hkv) * 128:].view(hkv, 128)
        cache.append_prefill(0, b, keys, vals[b])
        cache.lens[b] = m
    return case, want.view(n, hkv, 1, 128).expand(n, hkv, gsz, 128).reshape(n, hq * 128).contiguous()
