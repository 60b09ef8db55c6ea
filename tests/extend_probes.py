"""Inputs and references for crag_enc_extend_attention (tests/test_extend_gpu.py), in the style of decode_probes.py:
random ragged caches with NaN in every row behind the live ones, the fp32 formula, and one-key probes -- the cached plus
the new rows of a sequence hold keys that are all zero except key j, which is 16 x the rotated query of query row r, so
that every other softmax weight underflows to exactly 0 and out[r] must be V[j] bit for bit.

The cache is a one-layer KvCache, filled and read through its accessors (append_prefill, keys, values).  max_len is no
multiple of the tile, so a read past a slot's end would land in the NaN rows of the next kv head or slot.
(rotated() takes crag_enc_qk_norm_rope as the reference; test_row_probes_gpu.py pins the appended rows without it.)"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from decode_probes import BF, EPS, SCALE, rope_table

BLOCK = 32       # CRAG_EXTEND_BLOCK: query rows per workgroup
TILE = 32        # CRAG_EXTEND_TILE: keys per step of a workgroup
SPLIT = 512      # CRAG_EXTEND_SPLIT: keys per workgroup of a split query block
SPLIT_ROWS = 512  # CRAG_EXTEND_SPLIT_ROWS: a sequence with more new rows is never split
MARK = 7.0       # out is pre-filled with it; PAD rows behind the last sequence must keep it
PAD = 3
CACHE_LENS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 1000]     # includes TILE - 1, TILE, TILE + 1, 2 TILE +- 1
NEW_LENS = [1, 2, 31, 32, 33, 64, 65, 100]                                # includes BLOCK - 1, BLOCK, BLOCK + 1, 2 BLOCK +- 1


def pairs() -> List[Tuple[int, int]]:
    """45 (cache_len, new_len) pairs = 15 ragged calls of three: every cache length two or three times, every new length
    four or five times (13 and 8 are coprime, so the combinations differ); three chosen so that cache + new ends
    exactly on a tile, one short of it and one past it; and six around the key split: a block whose keys end exactly on
    SPLIT beside one that is one key past it, a second split of one key behind SPLIT - 1 and behind SPLIT cached rows,
    three splits, and SPLIT_ROWS new rows (split) beside SPLIT_ROWS + 1 (never split)."""
    out = [(CACHE_LENS[i % 13], NEW_LENS[i % 8]) for i in range(36)]
    out += [(31, 1), (63, 64), (32, 33)]
    return out + [(SPLIT - 32, 33), (SPLIT - 1, 1), (SPLIT, 1), (1000, 100), (100, SPLIT_ROWS), (100, SPLIT_ROWS + 1)]


@dataclass
class Case:
    hq: int
    hkv: int
    slots: List[int]
    news: List[int]
    qkv_new: torch.Tensor     # [sum(news), (hq + 2 hkv) * 128] bf16, device: the sequences' rows back to back
    q_w: torch.Tensor
    k_w: torch.Tensor
    cos_sin: torch.Tensor
    cache: object             # KvCache, one layer; cache.lens[slot] = what the slot holds now
    workspace: torch.Tensor

    def row0(self, b: int) -> int:
        return sum(self.news[:b])


def make_case(hq: int, hkv: int, lens: Sequence[int], news: Sequence[int], slots: Sequence[int], *, n_slots: int = 8,
              max_len: int = 1111, seed: int = 0, device=None) -> Case:
    """Random new rows; slot slots[b] holds lens[b] random keys / values, every other cache row is NaN."""
    from cadence_rag_amd.encoder import ops
    from cadence_rag_amd.encoder.generate import KvCache
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(sum(news), (hq + 2 * hkv) * 128, generator=g).to(BF).to(device)
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
    return Case(hq, hkv, list(slots), list(news), qkv, q_w, k_w, rope_table(max_len, device), cache,
                ops.extend_workspace(8, hq, sum(news), max_len, device))


def rotated(case: Case) -> torch.Tensor:
    """The new rows as crag_enc_qk_norm_rope leaves them at positions len + i (q and k normed + rotated, v raw).  Call
    BEFORE run()."""
    from cadence_rag_amd.encoder import ops
    out = case.qkv_new.clone()
    pos = torch.cat([torch.arange(case.cache.lens[s], case.cache.lens[s] + n, dtype=torch.int32)
                     for s, n in zip(case.slots, case.news)]).to(out.device)
    ops.qk_norm_rope(out, case.q_w, case.k_w, case.cos_sin, pos, case.hq, case.hkv, EPS)
    return out


def run(case: Case, seqs: Optional[Sequence[int]] = None, part: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """One extend call over the sequences `seqs` of the case (default all) behind what their slots hold now; `part` =
    (first, count) takes that range of every chosen sequence's new rows.  The cache lengths grow.  Returns out
    [rows + PAD, hq * 128], pre-filled with MARK."""
    from cadence_rag_amd.encoder import ops
    seqs = list(range(len(case.news))) if seqs is None else list(seqs)
    spans = [(case.row0(b) + (part[0] if part else 0), part[1] if part else case.news[b]) for b in seqs]
    rows = torch.cat([case.qkv_new[a:a + n] for a, n in spans]).contiguous()
    out = torch.full((rows.shape[0] + PAD, case.hq * 128), MARK, dtype=BF, device=rows.device)
    kc, vc = case.cache.layer(0)
    slots = [case.slots[b] for b in seqs]
    ops.extend_attention(rows, case.q_w, case.k_w, case.cos_sin, kc, vc, slots, [case.cache.lens[s] for s in slots],
                         [n for _, n in spans], out, case.hq, case.hkv, EPS, SCALE, case.workspace)
    for s, (_, n) in zip(slots, spans):
        case.cache.lens[s] += n
    torch.cuda.synchronize()
    return out


def reference(case: Case, rot: torch.Tensor) -> torch.Tensor:
    """fp32 on the CPU: softmax(q K^T / sqrt(128)) V over the slot's cached rows plus the new rows, causally.  Call
    BEFORE run()."""
    hq, hkv, gsz = case.hq, case.hkv, case.hq // case.hkv
    f = rot.float().cpu()
    out = torch.zeros(f.shape[0], hq, 128)
    for b, (slot, n) in enumerate(zip(case.slots, case.news)):
        m, a = case.cache.lens[slot], case.row0(b)
        q = f[a:a + n, : hq * 128].view(n, hq, 128)
        keys = torch.cat([case.cache.keys(0, slot).float().cpu(), f[a:a + n, hq * 128: (hq + hkv) * 128].view(n, hkv, 128)])
        vals = torch.cat([case.cache.values(0, slot).float().cpu(), f[a:a + n, (hq + hkv) * 128:].view(n, hkv, 128)])
        hidden = torch.arange(m + n)[None, :] > (m + torch.arange(n))[:, None]       # key k > position of row i
        for h in range(hq):
            s = (q[:, h] @ keys[:, h // gsz].T) * SCALE
            out[a:a + n, h] = torch.softmax(s.masked_fill(hidden, float("-inf")), dim=1) @ vals[:, h // gsz]
    return out.view(f.shape[0], hq * 128)


def one_key_case(hq: int, hkv: int, probes: Sequence[Tuple[int, int]], m: int, n: int, *, seed: int = 0, device=None):
    """len(probes) <= 8 sequences in slots 0.., each with m cached keys and n new rows (max_len = m + n).  Probe (r, j) of
    sequence b: the only non-zero key of the m + n is key j = 16 x the rotated query of new row r (all query heads of a
    kv head share one raw query).  A cached key (j < m) is planted; a new key (j >= m) is made by the kernel from raw
    k[j - m] = raw q[r] under k_norm = 16 x q_norm.  Every row of the RoPE table is the table's row 7, so that a query
    and a key of different positions are rotated alike and the new key is 16 x that query exactly.
    Returns (case, rows [n_probes] = the row of out that probe b speaks about, value [n_probes, hq * 128] bf16 = V[j])."""
    from cadence_rag_amd.encoder import ops
    from cadence_rag_amd.encoder.generate import KvCache
    g = torch.Generator().manual_seed(seed)
    ns, gsz = len(probes), hq // hkv
    q_kv = torch.randn(ns, n, hkv, 1, 128, generator=g).to(BF)
    k_raw = torch.zeros(ns, n, hkv, 128, dtype=BF)
    for b, (r, j) in enumerate(probes):
        if j >= m:
            k_raw[b, j - m] = q_kv[b, r, :, 0]
    v_raw = torch.randn(ns, n, hkv, 128, generator=g).to(BF)
    qkv = torch.cat([q_kv.expand(ns, n, hkv, gsz, 128).reshape(ns * n, hq * 128), k_raw.view(ns * n, hkv * 128),
                     v_raw.view(ns * n, hkv * 128)], dim=1).to(device)
    q_w = (1 + 0.1 * torch.randn(128, generator=g)).to(BF)
    k_w = (q_w.float() * 16).to(BF)          # exact: a power of two
    max_len = m + n
    cache = KvCache(1, 8, hkv, max_len, device)
    cache.k.fill_(float("nan"))
    cache.v.fill_(float("nan"))
    cos_sin = rope_table(8, device)[7:8].expand(max_len, 64, 2).contiguous()
    case = Case(hq, hkv, list(range(ns)), [n] * ns, qkv, q_w.to(device), k_w.to(device), cos_sin, cache,
                ops.extend_workspace(8, hq, ns * n, max_len, device))
    rot = rotated(case)                      # (the slots are empty: positions 0.., all rotated alike)
    vals = torch.randn(ns, m, hkv, 128, generator=g).to(BF).to(device)
    keys = torch.zeros(ns, m, hkv, 128, dtype=BF, device=device)
    want = torch.empty(ns, hkv, 128, dtype=BF, device=device)
    for b, (r, j) in enumerate(probes):
        if j < m:
            q_rot = rot[b * n + r, : hq * 128].view(hkv, gsz, 128)[:, 0]
            keys[b, j] = (q_rot.float() * 16).to(BF)
            want[b] = vals[b, j]
        else:
            want[b] = v_raw[b, j - m].to(device)
    for b in range(ns):
        if m:
            cache.append_prefill(0, b, keys[b], vals[b])
        cache.lens[b] = m
    rows = torch.tensor([b * n + r for b, (r, _) in enumerate(probes)], device=device)
    return case, rows, want.view(ns, hkv, 1, 128).expand(ns, hkv, gsz, 128).reshape(ns, hq * 128).contiguous()
