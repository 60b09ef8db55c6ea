"""Greedy autoregressive decoding with a KV cache on MI355X: the Qwen3 decoder (Qwen3Encoder's weights and layer
kernels) with a full-vocabulary head -- the in-process LLM behind /answer (cadence_rag_amd.answer).

  prefill(token_lists)  the general packed forward over the prompts (library GEMMs, qk_rope_vt, the causal flash
                        attention); every layer's normed + rotated keys and raw values are copied into the cache.
  step(tokens)          one new token per live sequence: per layer qkv, crag_enc_decode_attention (q/k-norm + RoPE of
                        the new row, append, attention over the cache), o, MLP; then crag_enc_lm_head (final norm, fp32
                        logits over the whole vocabulary, greedy token).
  extend(token_lists)   m new tokens behind the n a slot already holds: the new rows only, with
                        crag_enc_extend_attention (norm + RoPE, append, flash attention over the cache rows in place).
                        prefill, extend and step's library branch share one layer loop (_layers) and hand it their own
                        qkv projection + attention; step's small_gemm branch (the 4B widths) is a layer of its own.
  generate(...)         prefill + steps until a stop id or the token budget; every token comes from one _Picker, built
                        per call, which hides the four selection modes.  Greedy, or with sampling=SamplingParams
                        drawn on the device by crag_enc_sample (temperature, top-k, top-p, min-p; seeded).  With
                        reuse_prefix=True a prompt that begins with what its slot holds (plan_reuse) keeps those rows and extends.  With a
                        grammar (cadence_rag_amd.grammar.TokenGrammar) every token is picked by crag_enc_grammar_argmax
                        among the tokens the sequence's automaton state allows, on the logits prefill / extend / step
                        return; the states live on the device.  Under a grammar a sampled token is drawn among the
                        tokens the state allows, and crag_enc_grammar_advance moves the state behind it.
  generate_samples(...) n continuations of one prompt from one prefill: slots 1..n-1 are forked from slot 0
                        (KvCache.fork: no copy), and step reads a child's shared rows in its parent's slot through
                        crag_enc_decode_attention_shared, which loads every wholly shared 128-key split once for two
                        sequences of a parent.  generate's own token loop (_token_loop).
  step_rows(token_rows) step with several new tokens per sequence, at most 8 in all: a pending token and drafted ones
                        behind it, through crag_enc_decode_attention_rows.  generate(speculate=k) drafts by prompt
                        lookup (cadence_rag_amd.speculate), verifies the drafts in one such forward and keeps the
                        tokens the plain loop would have produced (_speculative_loop); off by default.
  logprobs=n            generate / generate_samples score every produced token with crag_enc_logprobs on the logits it
                        was picked from (last_logprobs: token, logprob, rank, the mass a grammar left allowed, the n most
                        likely ids); score(prompts, continuations) gives the same records for text it is handed.
  penalties=...         generate / generate_samples first run crag_enc_adjust_logits on every row a token is picked from
                        (cadence_rag_amd.penalties: repetition, presence and frequency penalties, the n-gram ban, a bias
                        list, min_new_tokens) over a token log the picker keeps on the device, and pick on the adjusted
                        rows in every mode; logprobs keeps scoring the raw logits.  Off by default: nothing is launched.

The cache layout ([layer][slot][kv head][max_len][128] bf16, keys and values apart) sits behind KvCache.keys / .values.
At most MAX_SEQS = 8 sequences decode at a time.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from ..grammar import KIND_STOP, TokenGrammar, TokenTable
from ..logprobs import TokenLogprob
from ..penalties import PenaltyParams, bias_list, exempt_words
from ..penalties import active as active_penalties
from ..sampling import SamplingParams
from ..speculate import MAX_SPECULATE, propose_drafts
from . import ops
from .qwen3 import QKV_ROW_CHUNK, PackedBatch, Qwen3Config, Qwen3Encoder

MAX_SEQS = 8
MAX_ROWS = 8             # CRAG_DECODE_MAX_ROWS: the rows of one step_rows -- pending tokens and drafts together
PREFIX_MIN_REUSE = 32    # one query block of the extend kernel: below it a plain prefill is no dearer
CHAT_SYSTEM = "<|im_start|>system\n{system}<|im_end|>\n"
CHAT_USER = "<|im_start|>user\n{user}<|im_end|>\n"
CHAT_ASSISTANT = "<|im_start|>assistant\n{assistant}<|im_end|>\n"
CHAT_GENERATE = "<|im_start|>assistant\n<think>\n\n</think>\n\n"


class PromptTooLong(ValueError):
    """A prompt does not leave room for the requested new tokens inside the context window."""


def plan_reuse(resident_ids: Sequence[int], prompt_ids: Sequence[int], min_reuse: int = PREFIX_MIN_REUSE) -> int:
    """How many leading cache rows of a slot that holds `resident_ids` serve `prompt_ids`: the length of the common
    token prefix, at most len(prompt_ids) - 1 (one row must be computed to get logits), and 0 when that is less than
    min_reuse."""
    keep, top = 0, min(len(resident_ids), len(prompt_ids) - 1)
    while keep < top and int(resident_ids[keep]) == int(prompt_ids[keep]):
        keep += 1
    return keep if keep >= max(int(min_reuse), 1) else 0


class KvCache:
    """Keys (normed, rotated) and raw values of every layer for n_slots sequences of up to max_len tokens.  `lens[slot]`
    (host) is the number of tokens a slot holds.

    Forks.  A slot can be a CHILD of another: its first shared[slot] logical rows are rows of slot parent[slot], never
    copied, and only the rows behind them are its own (crag_enc_decode_attention_shared reads both in place).  A slot
    that is not forked has parent[slot] == slot and shared[slot] == 0.  Chains are one deep: a parent is never a child.
    The one rule that keeps a child's rows valid: whatever shortens or overwrites rows of a slot that children still
    share (release(slot, keep): a prefill into it, a truncation below a child's shared length) empties those children
    -- lens 0, no longer forked.  Appending to a parent is free: its new rows lie behind every child's shared length."""

    def __init__(self, n_layers: int, n_slots: int, hkv: int, max_len: int, device) -> None:
        shape = (n_layers, n_slots, hkv, max_len, 128)
        self.k = torch.zeros(shape, dtype=torch.bfloat16, device=device)
        self.v = torch.zeros(shape, dtype=torch.bfloat16, device=device)
        self.n_slots, self.max_len = int(n_slots), int(max_len)
        self.lens: List[int] = [0] * n_slots
        self.parent: List[int] = list(range(n_slots))
        self.shared: List[int] = [0] * n_slots

    def layer(self, i: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The two [n_slots, hkv, max_len, 128] arrays crag_enc_decode_attention takes."""
        return self.k[i], self.v[i]

    def _rows(self, store: torch.Tensor, layer: int, slot: int) -> torch.Tensor:
        own = store[layer, slot, :, :self.lens[slot]].transpose(0, 1)
        if not self.forked(slot):
            return own
        n = self.shared[slot]
        return torch.cat([store[layer, self.parent[slot], :, :n].transpose(0, 1), own[n:]])

    def keys(self, layer: int, slot: int) -> torch.Tensor:
        """[len, hkv, 128]: the cached keys of a slot, token-major -- the logical rows: of a child the parent's first
        `shared` rows, then its own (a copy; of a slot that is not forked a view of the cache)."""
        return self._rows(self.k, layer, slot)

    def values(self, layer: int, slot: int) -> torch.Tensor:
        return self._rows(self.v, layer, slot)

    # -- forks (host only) ----------------------------------------------------------------------------------------
    def forked(self, slot: int) -> bool:
        return self.shared[slot] > 0 and self.parent[slot] != slot

    def children(self, slot: int) -> List[int]:
        return [c for c in range(self.n_slots) if self.forked(c) and self.parent[c] == slot]

    def unfork(self, slot: int) -> None:
        self.parent[slot], self.shared[slot] = slot, 0

    def release(self, slot: int, keep: int) -> None:
        """Rows keep.. of `slot` are about to change or go: the children that share any of them are emptied."""
        for c in self.children(slot):
            if self.shared[c] > keep:
                self.lens[c] = 0
                self.unfork(c)

    def fork(self, src: int, dst_slots: Sequence[int]) -> None:
        """Every slot of dst_slots becomes a child that holds what src holds, without a copy: lens = lens[src], shared =
        lens[src], parent = src -- or src's own parent when src is a child, which must then hold no row of its own.
        What a dst held is gone (its own children are emptied).  ValueError: dst == src, a duplicate dst, a dst outside
        the cache, a dst that is the parent of a live child other than the dsts themselves."""
        src, dsts = int(src), [int(d) for d in dst_slots]
        if not 0 <= src < self.n_slots or any(not 0 <= d < self.n_slots for d in dsts):
            raise ValueError(f"fork takes slots in 0..{self.n_slots - 1}")
        if src in dsts or len(set(dsts)) != len(dsts):
            raise ValueError("fork: every dst must be a slot of its own, and none the source")
        root = self.parent[src] if self.forked(src) else src
        if root != src and self.lens[src] > self.shared[src]:
            raise ValueError(f"fork: slot {src} is a child with rows of its own; only its parent's rows can be shared")
        for d in dsts:
            if d == root or any(c not in dsts and self.lens[c] > 0 for c in self.children(d)):
                raise ValueError(f"fork: slot {d} is the parent of a live child")
        for d in dsts:
            self.release(d, 0)
            self.lens[d] = self.lens[src]
            self.parent[d], self.shared[d] = (root, self.lens[src]) if self.lens[src] else (d, 0)

    def append_prefill(self, layer: int, slot: int, k_rows: torch.Tensor, v_rows: torch.Tensor) -> None:
        """k_rows / v_rows [n, hkv, 128]: a prompt's keys and values as crag_enc_qk_rope_vt left them in qkv -> rows
        0..n-1 of the slot (lens is set by the caller once every layer is in)."""
        n = k_rows.shape[0]
        self.k[layer, slot, :, :n].copy_(k_rows.transpose(0, 1))
        self.v[layer, slot, :, :n].copy_(v_rows.transpose(0, 1))


class _Picker:
    """The token selection of one generate() call over n prompts.  pick(rows, logits, greedy_tokens, step) -> the next
    token of the sequences `rows` (logits [len(rows), vocab]): greedy_tokens as they are (nothing is launched), drawn
    by ops.sample, the allowed greedy one by ops.grammar_argmax, or drawn among the allowed ones.  It holds the draws and
    streams per prompt, and under a grammar the tables and every prompt's automaton state on the device."""

    def __init__(self, gen: "Qwen3Generator", n: int, grammar: Optional[TokenGrammar], sampling, streams,
                 logprobs: Optional[int] = None, penalties=None, prompts: Sequence[Sequence[int]] = (),
                 max_new_tokens: int = 0, stop: Sequence[int] = (), exempt: Optional[Sequence[int]] = None) -> None:
        self.device = gen.device
        self.table = self.draws = None
        # penalties: every pick first runs ops.adjust_logits on the rows' logits and picks on the adjusted rows; the
        # picker then owns a token log on the device (the prompts, uploaded once, and every token it picks, appended
        # from the device tensor it was picked into) and the host lengths of its rows.  None or neutral: none of this.
        rules = [penalties] * n if penalties is None or isinstance(penalties, PenaltyParams) else list(penalties)
        if len(rules) != n or any(p is not None and not isinstance(p, PenaltyParams) for p in rules):
            raise ValueError("penalties takes one PenaltyParams, or one per prompt")
        self.rules: Optional[List[PenaltyParams]] = None
        if any(active_penalties(p) is not None for p in rules):
            if n > gen.max_seqs:
                raise ValueError(f"penalties take 1..{gen.max_seqs} prompts")
            self.rules = [p if p is not None else PenaltyParams() for p in rules]
            self.stop_ids = sorted({int(s) for s in stop})
            self.prompt_len = [len(p) for p in prompts]
            self.log_len = list(self.prompt_len)
            log = np.zeros((n, max(self.prompt_len) + int(max_new_tokens)), dtype=np.int32)
            for b, p in enumerate(prompts):
                log[b, :len(p)] = np.asarray(p, dtype=np.int32)
            self.log = torch.from_numpy(log).to(self.device)
            self.adjusted, self.adjust_ws = gen._adjust_buffers()
            self.exempt_bits = None if exempt is None else gen._exempt_bits(exempt)
            self.bias_key, self.bias_dev = None, (None, None)
        # logprobs = n_top: every pick is scored by ops.logprobs on the logits it was picked from; `scores` then holds the
        # TokenLogprob of every row of the last pick, and the token loops file those of the tokens they emit in `records`
        self.n_top = None if logprobs is None else _check_logprobs(logprobs, gen.cfg.vocab_size)
        self.scores: Optional[List[TokenLogprob]] = None
        self.records: Optional[List[List[TokenLogprob]]] = None if logprobs is None else [[] for _ in range(n)]
        if logprobs is not None and n > gen.max_seqs:
            raise ValueError(f"logprobs takes 1..{gen.max_seqs} prompts")
        if grammar is not None:
            self.table = grammar.table if grammar.table is not None else gen.token_table()
            if self.table.vocab != gen.cfg.vocab_size:
                raise ValueError(f"the grammar's token table holds {self.table.vocab} ids, the model {gen.cfg.vocab_size}")
            if n > gen.max_seqs:
                raise ValueError(f"generate takes 1..{gen.max_seqs} prompts")
        if sampling is not None:
            self.draws = [sampling] * n if isinstance(sampling, SamplingParams) else list(sampling)
            self.lanes = list(range(n)) if streams is None else [int(s) for s in streams]
            if n > gen.max_seqs or len(self.draws) != n or len(self.lanes) != n:
                raise ValueError(f"sampling takes 1..{gen.max_seqs} prompts, and one SamplingParams and one stream for each")
            if len({int(d.seed) for d in self.draws}) > 1:
                raise ValueError("the prompts of one call are drawn with one seed")
        if grammar is not None:
            self.tables = self.table.to(self.device) + grammar.dfa.to(self.device)
            self.state = torch.full((n,), int(grammar.dfa.start), dtype=torch.int32, device=self.device)

    def _draw(self, rows: List[int], logits: torch.Tensor, step: int, bits: Optional[torch.Tensor] = None) -> torch.Tensor:
        token = torch.empty(len(rows), dtype=torch.int32, device=self.device)
        return ops.sample(logits, [self.draws[b] for b in rows], step, [self.lanes[b] for b in rows], token,
                          allowed_bits=bits)

    def _adjust(self, rows: List[int], logits: torch.Tensor, step: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The rows' logits under their penalties (into the picker's scratch) and the greedy tokens on them.  step: how
        many ids every row has produced -- below min_new_tokens the stop ids are biased to -inf."""
        n, vocab = logits.shape
        lists = [bias_list(self.rules[b], step, self.stop_ids, vocab) for b in rows]
        bias = {}
        if any(lists):
            key = tuple(tuple(x) for x in lists)
            if key != self.bias_key:   # the lists change when a row passes min_new_tokens or the rows do: rarely
                flat = [e for x in lists for e in x]
                self.bias_key = key
                self.bias_dev = (torch.tensor([t for t, _ in flat], dtype=torch.int32).to(self.device),
                                 torch.tensor([v for _, v in flat], dtype=torch.float32).to(self.device))
            bias = dict(bias_ids=self.bias_dev[0], bias_values=self.bias_dev[1],
                        bias_offsets=np.concatenate([[0], np.cumsum([len(x) for x in lists])]).tolist())
        out = self.adjusted[:n]
        token = torch.empty(n, dtype=torch.int32, device=self.device)
        ops.adjust_logits(logits.contiguous(), out, self.log, rows, [self.prompt_len[b] for b in rows],
                          [self.log_len[b] for b in rows], [self.rules[b] for b in rows], token, self.adjust_ws,
                          exempt_bits=self.exempt_bits, **bias)
        return out, token

    def _append(self, rows: List[int], token: torch.Tensor) -> None:
        """The picked tokens go behind the rows' logs, device to device.  (A -1 or a stop id ends its sequence: whatever
        is appended for it is never read.)"""
        at = torch.tensor([rows, [self.log_len[b] for b in rows]], dtype=torch.int64).to(self.device)
        self.log.index_put_((at[0], at[1]), token)
        for b in rows:
            self.log_len[b] += 1

    def __call__(self, rows: List[int], logits: torch.Tensor, greedy_tokens: torch.Tensor, step: int) -> List[int]:
        raw = logits    # what logprobs scores: the model's own distribution, whatever picked the id
        if self.rules is not None:   # lm_head's greedy token is not valid under penalties: the kernel's is
            logits, greedy_tokens = self._adjust(rows, logits, step)
        token = self._pick(rows, logits, raw, greedy_tokens, step)
        if self.rules is not None:
            self._append(rows, token)
        return token.tolist()

    def _pick(self, rows: List[int], logits: torch.Tensor, raw: torch.Tensor, greedy_tokens: torch.Tensor, step: int
              ) -> torch.Tensor:
        if self.table is None:
            token = greedy_tokens if self.draws is None else self._draw(rows, logits, step)
            if self.n_top is not None:
                self.scores = score_rows(raw, token, self.n_top)
            return token
        idx = torch.tensor(rows, dtype=torch.int64).to(self.device)
        cur = self.state.index_select(0, idx)      # the states of `rows`: they move on behind the chosen tokens
        token = torch.empty(len(rows), dtype=torch.int32, device=self.device)
        bits = None
        if self.draws is not None or self.n_top is not None:
            bits = torch.empty(len(rows), (self.table.vocab + 31) // 32, dtype=torch.int32, device=self.device)
        if self.draws is None:
            ops.grammar_argmax(logits, *self.tables, cur, token, allowed_bits=bits)
        else:   # grammar_argmax hands out the bits on a copy of the states; its own token is dropped
            ops.grammar_argmax(logits, *self.tables, cur.clone(), token, allowed_bits=bits)
            token = self._draw(rows, logits, step, bits)
            ops.grammar_advance(*self.tables[:5], cur, token)
        self.state.index_copy_(0, idx, cur)
        if self.n_top is not None:   # the bits grammar_argmax handed out: the mass the automaton left allowed
            self.scores = score_rows(raw, token, self.n_top, bits)
        return token

    def file(self, b: int, k: int) -> None:
        """The token loop emitted row k of the last pick as a token of prompt b: its record is kept."""
        if self.records is not None:
            self.records[b].append(self.scores[k])


def _check_logprobs(logprobs, vocab: int) -> int:
    if isinstance(logprobs, bool) or int(logprobs) != logprobs or not 0 <= int(logprobs) <= min(ops.MAX_TOP_LOGPROBS, vocab):
        raise ValueError(f"logprobs must be None or an integer in 0..{min(ops.MAX_TOP_LOGPROBS, vocab)} (got {logprobs!r})")
    return int(logprobs)


def score_rows(logits: torch.Tensor, token: torch.Tensor, n_top: int, bits: Optional[torch.Tensor] = None
               ) -> List[TokenLogprob]:
    """One TokenLogprob per row of logits [n <= 8, vocab] for the ids token [n] (int32, device): ops.logprobs, its
    float outputs in one buffer and its integer outputs in another, so that two copies bring everything to the host.
    bits: the allowed flags of a grammar; the records then carry allowed_logmass = lse_allowed - lse_all."""
    n, dev = logits.shape[0], logits.device
    f = torch.empty(n * (3 + n_top), dtype=torch.float32, device=dev)
    i = torch.empty(n * (1 + n_top), dtype=torch.int32, device=dev)
    top_lp = f[3 * n:].view(n, n_top) if n_top else None
    top_id = i[n:].view(n, n_top) if n_top else None
    ops.logprobs(logits, token.contiguous(), f[:n], allowed_bits=bits, lse_all=f[n:2 * n],
                 lse_allowed=f[2 * n:3 * n] if bits is not None else None, rank=i[:n], top_id=top_id, top_logprob=top_lp)
    ids, fh, ih = token.tolist(), f.tolist(), i.tolist()
    out = []
    for r in range(n):
        top = [(ih[n + r * n_top + k], fh[3 * n + r * n_top + k]) for k in range(n_top)]
        mass = fh[2 * n + r] - fh[n + r] if bits is not None else None
        out.append(TokenLogprob(int(ids[r]), fh[r], ih[r], mass, top))
    return out


class Qwen3Generator:
    """generate(prompts, max_new_tokens, stop_ids) -> new token ids of every prompt, on one GPU and one stream."""

    supports_grammar = True   # generate / generate_text take grammar=TokenGrammar (answer.py asks before passing one)
    supports_sampling = True  # ... and sampling=SamplingParams
    supports_samples = True   # generate_text_samples: n replies from one prefill
    supports_speculation = True   # ... and speculate=k: up to k prompt-lookup drafts verified per forward
    supports_logprobs = True      # ... and logprobs=n: last_logprobs holds a TokenLogprob per produced token
    supports_penalties = True     # ... and penalties=PenaltyParams, penalty_exempt=ids: repetition control

    def __init__(self, encoder: Qwen3Encoder, lm_head: torch.Tensor, tokenizer=None, *, max_context: Optional[int] = None,
                 max_seqs: int = MAX_SEQS, model_id: Optional[str] = None, prefix_cache: bool = False) -> None:
        c = encoder.cfg
        if c.head_dim != 128 or c.num_heads % c.num_kv_heads or c.num_heads // c.num_kv_heads not in (2, 4):
            raise ValueError("the decode attention kernel is built for head_dim 128 and 2 or 4 query heads per kv head")
        if tuple(lm_head.shape) != (c.vocab_size, c.hidden_size):
            raise ValueError(f"lm_head must be [{c.vocab_size}, {c.hidden_size}]")
        if not 1 <= int(max_seqs) <= MAX_SEQS:
            raise ValueError(f"max_seqs must be in 1..{MAX_SEQS}")
        self.encoder = encoder
        self.cfg = c
        self.device = encoder.device
        self.max_context = int(max_context or c.max_length)
        if self.max_context > c.max_length:
            raise ValueError(f"max_context {self.max_context} exceeds the encoder's RoPE table ({c.max_length} positions)")
        # a tied model passes embed_tokens itself: the same storage, no copy
        self.lm_head = lm_head if (lm_head.device == self.device and lm_head.dtype == torch.bfloat16
                                   and lm_head.is_contiguous()) else \
            lm_head.to(device=self.device, dtype=torch.bfloat16).contiguous()
        self.tokenizer = tokenizer
        self.model_id = model_id or c.model_id
        self.max_seqs = int(max_seqs)
        self.cache = KvCache(c.num_layers, self.max_seqs, c.num_kv_heads, self.max_context, self.device)
        self._workspace = ops.decode_workspace(self.max_seqs, c.num_heads, self.max_context, self.device)
        self._extend_ws: Optional[torch.Tensor] = None   # extend's scratch: grows to the largest call
        self._rows_ws: Optional[torch.Tensor] = None     # step_rows' scratch for MAX_ROWS rows: made on first use
        self.live: List[int] = []          # slots of the sequences the next step() advances
        self.tokens: List[List[int]] = [[] for _ in range(self.max_seqs)]   # the token ids every slot holds
        self.prefix_cache = bool(prefix_cache)   # generate_text reuses a slot's rows (generate(reuse_prefix=True))
        self.last_reuse: Optional[Dict[str, List[int]]] = None   # per prompt of the last generate(reuse_prefix=True)
        self.last_grammar: Optional[Dict[str, List[bool]]] = None   # per prompt of the last generate(grammar=...)
        self.last_speculation: Optional[Dict[str, object]] = None   # of the last generate(speculate=k > 0)
        self.last_logprobs: Optional[List[List[TokenLogprob]]] = None   # per prompt of the last generate(logprobs=n)
        self.last_score_logits: Optional[List[torch.Tensor]] = None     # of the last score(keep_logits=True)
        self._token_table: Optional[TokenTable] = None   # the vocabulary's bytes: built once, its tensors stay in HBM
        self.force_library = False         # tests: keep the 4B widths off the small_gemm path
        self.last_path = ""

    # -- construction ---------------------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, path: str, device: Optional[torch.device] = None, max_context: int = 8192, *,
                        max_seqs: int = MAX_SEQS, model_id: Optional[str] = None, prefix_cache: bool = False
                        ) -> "Qwen3Generator":
        """A local *ForCausalLM checkpoint directory (config.json, *.safetensors, tokenizer files; nothing is fetched),
        lm_head tied to embed_tokens or not."""
        import json
        from pathlib import Path

        from safetensors.torch import load_file
        from transformers import AutoTokenizer
        root = Path(path)
        hf = json.loads((root / "config.json").read_text())
        rope = hf.get("rope_theta") or (hf.get("rope_parameters") or {}).get("rope_theta", 1_000_000.0)
        cfg = Qwen3Config(hidden_size=hf["hidden_size"], num_layers=hf["num_hidden_layers"],
                          num_heads=hf["num_attention_heads"], num_kv_heads=hf["num_key_value_heads"],
                          head_dim=hf.get("head_dim", 128), intermediate_size=hf["intermediate_size"],
                          vocab_size=hf["vocab_size"], rms_norm_eps=hf.get("rms_norm_eps", 1e-6), rope_theta=rope,
                          max_length=int(max_context), out_dim=min(1024, hf["hidden_size"]), pooling="last",
                          model_id=model_id or hf.get("_name_or_path") or str(root.name))
        tokenizer = AutoTokenizer.from_pretrained(str(root), local_files_only=True)
        files = sorted(root.glob("*.safetensors"))
        if not files:
            raise FileNotFoundError(f"no *.safetensors under {root}")
        sd: Dict[str, torch.Tensor] = {}
        for f in files:
            sd.update(load_file(str(f)))
        prefix = "model." if any(k.startswith("model.") for k in sd) else ""
        tied = hf.get("tie_word_embeddings", False) or "lm_head.weight" not in sd
        if tied and not hf.get("tie_word_embeddings", False):
            raise ValueError(f"{root}: no lm_head.weight and the config does not tie it to embed_tokens")
        head = None if tied else sd.pop("lm_head.weight")
        sd.pop("lm_head.weight", None)
        enc = Qwen3Encoder.from_state_dict(cfg, sd, device, prefix=prefix)
        enc.tokenizer = tokenizer
        return cls(enc, enc.embed if tied else head, tokenizer, max_context=max_context, max_seqs=max_seqs,
                   model_id=cfg.model_id, prefix_cache=prefix_cache)

    # -- prompts --------------------------------------------------------------------------------------------------
    def chat_ids(self, messages: Sequence[Dict[str, str]]) -> List[int]:
        """Token ids of a chat (system / user / assistant turns) ending in the assistant's opening: the tokenizer's own
        chat template when it has one, otherwise the ChatML text the reranker writes by hand."""
        tok = self._tokenizer()
        if getattr(tok, "chat_template", None):
            text = tok.apply_chat_template(list(messages), tokenize=False, add_generation_prompt=True)
        else:
            forms = {"system": CHAT_SYSTEM, "user": CHAT_USER, "assistant": CHAT_ASSISTANT}
            text = "".join(forms[m["role"]].format(**{m["role"]: m["content"]}) for m in messages) + CHAT_GENERATE
        return tok.encode(text, add_special_tokens=False)

    def stop_ids(self) -> List[int]:
        tok = self._tokenizer()
        ids = []
        vocab = tok.get_vocab()
        if "<|im_end|>" in vocab:
            ids.append(int(vocab["<|im_end|>"]))
        if getattr(tok, "eos_token_id", None) is not None:
            ids.append(int(tok.eos_token_id))
        return sorted(set(ids))

    def token_table(self) -> TokenTable:
        """The bytes and kinds of the whole vocabulary (the model's, which may be padded beyond the tokenizer's), the
        stop ids as stop tokens: what a TokenGrammar without a table of its own decodes with."""
        if self._token_table is None:
            self._token_table = TokenTable.from_tokenizer(self._tokenizer(), self.stop_ids(), self.cfg.vocab_size)
        return self._token_table

    # -- repetition control: what a _Picker with penalties borrows --------------------------------------------------
    def _adjust_buffers(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(the adjusted rows [MAX_ROWS, vocab] fp32, ops.adjust_logits' workspace): made on the first call with
        penalties, kept for the later ones."""
        bufs = self.__dict__.get("_adjust_bufs")
        if bufs is None:
            bufs = self._adjust_bufs = (torch.empty(MAX_ROWS, self.cfg.vocab_size, dtype=torch.float32, device=self.device),
                                        ops.adjust_workspace(MAX_ROWS, self.cfg.vocab_size, self.device))
        return bufs

    def _exempt_bits(self, ids: Sequence[int]) -> torch.Tensor:
        """The exempt ids as the kernel's bit mask on the device; the last list's mask is kept (/answer passes one)."""
        key = np.unique(np.asarray(ids, dtype=np.int64)).tobytes()
        held = self.__dict__.get("_exempt_held")
        if held is None or held[0] != key:
            words = exempt_words(np.frombuffer(key, dtype=np.int64), self.cfg.vocab_size)
            held = self._exempt_held = (key, torch.from_numpy(words.view(np.int32)).to(self.device))
        return held[1]

    def _tokenizer(self):
        if self.tokenizer is None:
            raise RuntimeError("no tokenizer loaded (Qwen3Generator.from_pretrained, or pass one)")
        return self.tokenizer

    # -- forward --------------------------------------------------------------------------------------------------
    def _head(self, hidden: torch.Tensor, delta: Optional[torch.Tensor], banned=None) -> Tuple[torch.Tensor, torch.Tensor]:
        n = hidden.shape[0]
        logits = torch.empty(n, self.cfg.vocab_size, dtype=torch.float32, device=self.device)
        token = torch.empty(n, dtype=torch.int32, device=self.device)
        ops.lm_head(hidden, self.encoder.final_norm, self.lm_head, logits, token, self.cfg.rms_norm_eps, delta=delta,
                    banned=banned)
        return logits, token

    def _check_slots(self, what: str, n: int, slots: Optional[Sequence[int]]) -> List[int]:
        slots = list(range(n)) if slots is None else [int(s) for s in slots]
        if not 1 <= n <= self.max_seqs or len(slots) != n or len(set(slots)) != n or \
                any(not 0 <= s < self.max_seqs for s in slots):
            raise ValueError(what % self.max_seqs)
        return slots

    def _embed(self, token_lists: Sequence[Sequence[int]]) -> torch.Tensor:
        ids = torch.from_numpy(np.concatenate([np.asarray(tl, dtype=np.int32) for tl in token_lists])).to(self.device)
        x = torch.empty(ids.numel(), self.cfg.hidden_size, dtype=torch.bfloat16, device=self.device)
        ops.embed_gather(ids, self.encoder.embed, x)
        return x

    def _layers(self, x: torch.Tensor, project_and_attend) -> Tuple[torch.Tensor, torch.Tensor]:
        """The decoder layers over the embedded rows x with library GEMMs: rmsnorm, project_and_attend(i, L, normed) ->
        the attention output [rows, q_size] (the caller's qkv projection and attention against layer i), o, rmsnorm,
        gate_up, swiglu, down.  Returns (resid, delta): the hidden state is their sum."""
        c = self.cfg
        resid, normed = torch.empty_like(x), torch.empty_like(x)
        act = torch.empty(x.shape[0], c.intermediate_size, dtype=x.dtype, device=x.device)
        delta: Optional[torch.Tensor] = None
        for i, L in enumerate(self.encoder.layers):
            if i == 0:
                ops.rmsnorm(x, L["ln1"], normed, c.rms_norm_eps, residual_in=None, residual_out=None)
                resid.copy_(x)
            else:
                ops.rmsnorm(delta, L["ln1"], normed, c.rms_norm_eps, residual_in=resid, residual_out=resid)
            delta = F.linear(project_and_attend(i, L, normed), L["o"])
            ops.rmsnorm(delta, L["ln2"], normed, c.rms_norm_eps, residual_in=resid, residual_out=resid)
            ops.swiglu(F.linear(normed, L["gate_up"]), act)
            delta = F.linear(act, L["down"])
        return resid, delta

    @torch.no_grad()
    def prefill(self, token_lists: Sequence[Sequence[int]], slots: Optional[Sequence[int]] = None) -> torch.Tensor:
        """Fills slot slots[b] (default b) with prompt b and makes these the live sequences.  Returns the last-token
        logits [n, vocab] fp32 on the device; .last_tokens holds their greedy tokens (int32 [n], device)."""
        slots = self._check_slots("prefill takes 1..%d prompts, each in a slot of its own", len(token_lists), slots)
        resid, delta, batch = self._prefill_rows(token_lists, slots)
        logits, self.last_tokens = self._head(resid.index_select(0, batch.last_tok),
                                              delta.index_select(0, batch.last_tok))
        return logits

    def _prefill_rows(self, token_lists: Sequence[Sequence[int]], slots: List[int]):
        """prefill's layers over every row of the prompts: fills the slots, makes them the live sequences and returns
        (resid, delta, batch) -- the hidden state of packed row i is resid[i] + delta[i] (prefill heads the last rows,
        score the rows that predict a continuation)."""
        c, enc, dev, bf = self.cfg, self.encoder, self.device, torch.bfloat16
        lens = [len(tl) for tl in token_lists]
        if min(lens) <= 0:
            raise ValueError("every prompt needs at least one token")
        if max(lens) >= self.max_context:
            raise PromptTooLong(f"a prompt of {max(lens)} tokens leaves no room in a context of {self.max_context}")
        for slot in slots:   # rows 0.. of the slot are overwritten: it is nobody's child and nobody's parent afterwards
            self.cache.unfork(slot)
            self.cache.release(slot, 0)
        batch = PackedBatch.build(lens, dev)
        t = batch.n_tokens
        x = self._embed(token_lists)
        qkv_buf = torch.zeros(t + 32, c.q_size + 2 * c.kv_size, dtype=bf, device=dev)  # attention reads up to 31 rows past T
        qkv = qkv_buf[:t]
        vt = torch.empty(c.num_kv_heads, c.head_dim, batch.t_pad, dtype=bf, device=dev)
        attn = torch.empty(t, c.q_size, dtype=bf, device=dev)
        scale = 1.0 / math.sqrt(c.head_dim)
        starts = np.concatenate([[0], np.cumsum(lens)])

        def attend(i, L, normed):
            for lo in range(0, t, QKV_ROW_CHUNK):
                hi = min(t, lo + QKV_ROW_CHUNK)
                torch.matmul(normed[lo:hi], L["qkv"].t(), out=qkv[lo:hi])
            ops.qk_rope_vt(qkv_buf, L["q_norm"], L["k_norm"], enc._cos_sin, batch.positions, c.num_heads, c.num_kv_heads,
                           c.rms_norm_eps, vt, batch.tok_of_pad)
            for b, slot in enumerate(slots):   # KV append: the normed + rotated keys and the raw values of the prompt
                rows = qkv[int(starts[b]):int(starts[b + 1])]
                self.cache.append_prefill(i, slot, rows[:, c.q_size:c.q_size + c.kv_size].view(-1, c.num_kv_heads, 128),
                                          rows[:, c.q_size + c.kv_size:].view(-1, c.num_kv_heads, 128))
            ops.attention(qkv_buf, vt, attn, batch.cu, batch.cu_pad, batch.blk_seq, batch.blk_q0, c.num_heads,
                          c.num_kv_heads, scale)
            return attn

        resid, delta = self._layers(x, attend)
        for slot, m, tl in zip(slots, lens, token_lists):
            self.cache.lens[slot] = m
            self.tokens[slot] = [int(x) for x in tl]
        self.live = list(slots)
        return resid, delta, batch

    @torch.no_grad()
    def extend(self, token_lists: Sequence[Sequence[int]], slots: Optional[Sequence[int]] = None) -> torch.Tensor:
        """Appends token_lists[b] to slot slots[b] (default b) behind the cache.lens[slot] tokens it holds -- an empty
        slot is allowed -- and makes these the live sequences.  prefill's layers over the new rows only, with
        crag_enc_extend_attention in the place of qk_rope_vt + the cache copies + the packed attention.  Returns the
        logits of every sequence's last new row [n, vocab] fp32 on the device; .last_tokens holds their greedy tokens."""
        c, enc, dev, bf = self.cfg, self.encoder, self.device, torch.bfloat16
        n = len(token_lists)
        slots = self._check_slots("extend takes 1..%d token lists, each for a slot of its own", n, slots)
        news = [len(tl) for tl in token_lists]
        if min(news) <= 0:
            raise ValueError("every sequence needs at least one new token")
        if any(self.cache.forked(s) for s in slots):
            raise ValueError("extend cannot continue a forked slot: the extend kernel reads no parent")
        held = [self.cache.lens[s] for s in slots]
        full = max(h + m for h, m in zip(held, news))
        if full >= self.max_context:
            raise PromptTooLong(f"a sequence of {full} tokens leaves no room in a context of {self.max_context}")
        t = sum(news)
        need = ops.extend_workspace_bytes(n, c.num_heads, t, full)   # the rotated queries, the key splits' partials
        if self._extend_ws is None or self._extend_ws.numel() < need:
            self._extend_ws = torch.empty(need, dtype=torch.uint8, device=dev)
        x = self._embed(token_lists)
        qkv = torch.empty(t, c.q_size + 2 * c.kv_size, dtype=bf, device=dev)
        attn = torch.empty(t, c.q_size, dtype=bf, device=dev)
        scale = 1.0 / math.sqrt(c.head_dim)

        def attend(i, L, normed):
            for lo in range(0, t, QKV_ROW_CHUNK):
                hi = min(t, lo + QKV_ROW_CHUNK)
                torch.matmul(normed[lo:hi], L["qkv"].t(), out=qkv[lo:hi])
            ops.extend_attention(qkv, L["q_norm"], L["k_norm"], enc._cos_sin, *self.cache.layer(i), slots, held, news, attn,
                                 c.num_heads, c.num_kv_heads, c.rms_norm_eps, scale, self._extend_ws)
            return attn

        resid, delta = self._layers(x, attend)
        for slot, m, tl in zip(slots, news, token_lists):
            self._forget_stale(slot)
            self.cache.lens[slot] += m
            self.tokens[slot].extend(int(x) for x in tl)
        self.live = list(slots)
        last = torch.from_numpy(np.cumsum(news) - 1).to(dev)
        logits, self.last_tokens = self._head(resid.index_select(0, last), delta.index_select(0, last))
        return logits

    # -- what the slots hold ---------------------------------------------------------------------------------------
    def _forget_stale(self, slot: int) -> None:
        """A caller that set cache.lens by hand has left the id list behind: such a slot's ids are unknown (-1 matches
        no token, so nothing of it is ever reused)."""
        if len(self.tokens[slot]) != self.cache.lens[slot]:
            self.tokens[slot] = [-1] * self.cache.lens[slot]

    def resident(self, slot: int) -> List[int]:
        """The token ids slot holds, one per cache row."""
        self._forget_stale(slot)
        return self.tokens[slot]

    def truncate(self, slot: int, n: int) -> None:
        """Shortens a slot to its first n tokens.  Host only: rows behind cache.lens are never read and are overwritten
        by the next append."""
        n = int(n)
        if not 0 <= n <= self.cache.lens[slot]:
            raise ValueError(f"slot {slot} holds {self.cache.lens[slot]} tokens: cannot truncate to {n}")
        self._forget_stale(slot)
        self.cache.release(slot, n)      # children that share rows behind n are emptied
        self.cache.lens[slot] = n
        if self.cache.forked(slot):
            self.cache.shared[slot] = min(self.cache.shared[slot], n)
            if n == 0:
                self.cache.unfork(slot)
        del self.tokens[slot][n:]

    @torch.no_grad()
    def step(self, tokens: Sequence[int], slots: Optional[Sequence[int]] = None, banned: Optional[torch.Tensor] = None
             ) -> Tuple[torch.Tensor, torch.Tensor]:
        """One new token per sequence (slots: default the live ones, in order).  Returns (next tokens int32 [n], logits
        [n, vocab] fp32), both on the device; the cache of every slot grows by one."""
        c, enc, dev, bf = self.cfg, self.encoder, self.device, torch.bfloat16
        slots = list(self.live) if slots is None else [int(s) for s in slots]
        n = len(slots)
        if n == 0 or len(tokens) != n:
            raise ValueError("step needs one token per live sequence")
        lens = [self.cache.lens[s] for s in slots]
        if max(lens) >= self.max_context:
            raise PromptTooLong(f"a sequence of {max(lens)} tokens has filled the context of {self.max_context}")
        ids = torch.tensor([int(t) for t in tokens], dtype=torch.int32).to(dev)
        scale = 1.0 / math.sqrt(c.head_dim)
        width = c.q_size + 2 * c.kv_size
        if any(self.cache.forked(s) for s in slots):   # a child reads its parent's rows in place
            parents, shared = [self.cache.parent[s] for s in slots], [self.cache.shared[s] for s in slots]

            def attention(qkv, L, kc, vc):
                ops.decode_attention_shared(qkv, L["q_norm"], L["k_norm"], enc._cos_sin, kc, vc, slots, lens, parents,
                                            shared, attn, c.num_heads, c.num_kv_heads, c.rms_norm_eps, scale,
                                            self._workspace)
        else:
            def attention(qkv, L, kc, vc):
                ops.decode_attention(qkv, L["q_norm"], L["k_norm"], enc._cos_sin, kc, vc, slots, lens, attn, c.num_heads,
                                     c.num_kv_heads, c.rms_norm_eps, scale, self._workspace)
        skinny = None if self.force_library else enc._skinny_weights()
        if skinny is not None and not enc._skinny_v1:
            # the five-launch layer of Qwen3Encoder._forward_small_rows at 16 padded rows, the decode attention in the middle
            self.last_path = "small_gemm"
            bufs = self.__dict__.get("_small_bufs")
            if bufs is None:
                # allocated once and zeroed once: the kernels store the n live rows only, so the padding rows hold zeros
                # or the finite rows of an earlier, larger step -- and a row of a GEMM depends on no other row
                z = lambda cols: torch.zeros(16, cols, dtype=bf, device=dev)   # noqa: E731
                bufs = self._small_bufs = tuple(z(cols) for cols in (c.hidden_size,) * 5 + (width, c.q_size,
                                                                                            c.intermediate_size))
            res_a, res_b, delta_o, delta_d, delta0, qkv, attn, act = bufs
            ops.embed_gather(ids, enc.embed, res_a[:n])
            for i, L in enumerate(enc.layers):
                W = skinny[i]
                kc, vc = self.cache.layer(i)
                ops.small_gemm(res_a, W["qkv"], qkv, n, width, 12, delta=delta0 if i == 0 else delta_d, norm_w=L["ln1"],
                               res_out=res_b, eps=c.rms_norm_eps)
                attention(qkv, L, kc, vc)
                ops.small_gemm(attn, W["o"], delta_o, n, c.hidden_size, 10)
                ops.small_gemm(res_b, W["gate_up"], act, n, 2 * c.intermediate_size, 16, swiglu=True, delta=delta_o,
                               norm_w=L["ln2"], res_out=res_a, eps=c.rms_norm_eps)
                ops.small_gemm(act, W["down"], delta_d, n, c.hidden_size, 10)
            hidden, delta = res_a[:n], delta_d[:n]
        else:
            self.last_path = "library"
            x = torch.empty(n, c.hidden_size, dtype=bf, device=dev)
            ops.embed_gather(ids, enc.embed, x)
            attn = torch.empty(n, c.q_size, dtype=bf, device=dev)

            def attend(i, L, normed):
                attention(F.linear(normed, L["qkv"]), L, *self.cache.layer(i))
                return attn

            hidden, delta = self._layers(x, attend)
        for s, tok in zip(slots, tokens):
            self._forget_stale(s)
            self.cache.lens[s] += 1
            self.tokens[s].append(int(tok))
        logits, token = self._head(hidden, delta, banned)
        return token, logits

    @torch.no_grad()
    def step_rows(self, token_rows: Sequence[Sequence[int]], slots: Optional[Sequence[int]] = None,
                  banned: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """step with SEVERAL new tokens per sequence: token_rows[b] (at least one id) goes behind what slot slots[b]
        (default the live ones, in order) holds, R = the total number of ids <= MAX_ROWS.  Returns (next tokens int32
        [R], logits [R, vocab] fp32) in call order: row i of a sequence is what step would return after feeding it the
        ids 0..i one at a time -- to the bit on the small_gemm path, where every row of a GEMM, of lm_head and of
        crag_enc_decode_attention_rows depends on that row alone.  The cache of every slot grows by its row count; the
        caller cuts back what it does not keep (truncate).  Forked slots are allowed."""
        c, enc, dev, bf = self.cfg, self.encoder, self.device, torch.bfloat16
        slots = list(self.live) if slots is None else [int(s) for s in slots]
        news = [len(row) for row in token_rows]
        n = sum(news)
        if not slots or len(token_rows) != len(slots) or min(news) < 1 or n > MAX_ROWS:
            raise ValueError(f"step_rows needs at least one token per live sequence and at most {MAX_ROWS} in all")
        lens = [self.cache.lens[s] for s in slots]
        full = max(m + r for m, r in zip(lens, news))
        if full > self.max_context:
            raise PromptTooLong(f"a sequence of {full} tokens does not fit the context of {self.max_context}")
        if self._rows_ws is None:   # the constructor's scratch holds max_seqs rows
            self._rows_ws = self._workspace if self.max_seqs >= MAX_ROWS else \
                ops.decode_workspace(MAX_ROWS, c.num_heads, self.max_context, dev)
        ids = torch.tensor([int(t) for row in token_rows for t in row], dtype=torch.int32).to(dev)
        scale = 1.0 / math.sqrt(c.head_dim)
        width = c.q_size + 2 * c.kv_size
        forked = any(self.cache.forked(s) for s in slots)
        parents = [self.cache.parent[s] for s in slots] if forked else None
        shared = [self.cache.shared[s] for s in slots] if forked else None

        def attention(qkv, L, kc, vc):
            ops.decode_attention_rows(qkv, L["q_norm"], L["k_norm"], enc._cos_sin, kc, vc, slots, lens, news, attn,
                                      c.num_heads, c.num_kv_heads, c.rms_norm_eps, scale, self._rows_ws, parents=parents,
                                      shared_len=shared)
        skinny = None if self.force_library else enc._skinny_weights()
        if skinny is not None and not enc._skinny_v1:
            # step's small_gemm layer: the same launches over n rows of the same 16 padded ones
            self.last_path = "small_gemm"
            bufs = self.__dict__.get("_small_bufs")
            if bufs is None:
                z = lambda cols: torch.zeros(16, cols, dtype=bf, device=dev)   # noqa: E731
                bufs = self._small_bufs = tuple(z(cols) for cols in (c.hidden_size,) * 5 + (width, c.q_size,
                                                                                            c.intermediate_size))
            res_a, res_b, delta_o, delta_d, delta0, qkv, attn, act = bufs
            ops.embed_gather(ids, enc.embed, res_a[:n])
            for i, L in enumerate(enc.layers):
                W = skinny[i]
                kc, vc = self.cache.layer(i)
                ops.small_gemm(res_a, W["qkv"], qkv, n, width, 12, delta=delta0 if i == 0 else delta_d, norm_w=L["ln1"],
                               res_out=res_b, eps=c.rms_norm_eps)
                attention(qkv, L, kc, vc)
                ops.small_gemm(attn, W["o"], delta_o, n, c.hidden_size, 10)
                ops.small_gemm(res_b, W["gate_up"], act, n, 2 * c.intermediate_size, 16, swiglu=True, delta=delta_o,
                               norm_w=L["ln2"], res_out=res_a, eps=c.rms_norm_eps)
                ops.small_gemm(act, W["down"], delta_d, n, c.hidden_size, 10)
            hidden, delta = res_a[:n], delta_d[:n]
        else:
            self.last_path = "library"
            x = torch.empty(n, c.hidden_size, dtype=bf, device=dev)
            ops.embed_gather(ids, enc.embed, x)
            attn = torch.empty(n, c.q_size, dtype=bf, device=dev)

            def attend(i, L, normed):
                attention(F.linear(normed, L["qkv"]), L, *self.cache.layer(i))
                return attn

            hidden, delta = self._layers(x, attend)
        for s, row in zip(slots, token_rows):
            self._forget_stale(s)
            self.cache.lens[s] += len(row)
            self.tokens[s].extend(int(t) for t in row)
        logits, token = self._head(hidden, delta, banned)
        return token, logits

    @torch.no_grad()
    def generate(self, prompts: Sequence[Sequence[int]], max_new_tokens: int, stop_ids: Sequence[int] = (),
                 reuse_prefix: bool = False, grammar: Optional[TokenGrammar] = None,
                 sampling=None, streams: Optional[Sequence[int]] = None, speculate: int = 0,
                 drafter=None, logprobs: Optional[int] = None, penalties=None,
                 penalty_exempt: Optional[Sequence[int]] = None) -> List[List[int]]:
        """Greedy continuation of every prompt (token ids): at most max_new_tokens ids each, ending before the first
        stop id.  A prompt longer than max_context - max_new_tokens raises PromptTooLong (a ValueError): the caller
        shortens its prompt, nothing is truncated here.
        reuse_prefix: prompt b is planned against what slot b holds (plan_reuse).  If no slot can keep anything the call
        is the plain prefill; otherwise every slot is cut to what it keeps and the rests go through one extend().
        last_reuse = {"reused": [...], "computed": [...]} then holds the tokens per prompt (None without reuse_prefix).
        grammar: every prompt gets an automaton state on the device, starting at grammar.dfa.start; every token -- the
        first one too -- is the greedy one among the tokens that state allows (ops.grammar_argmax).  A sequence then also
        ends at a stop token of the grammar's table, which the automaton allows in accepting states only, and at -1
        (nothing allowed).  last_grammar = {"accepted": [...]}: whether each sequence ended on such a stop token (None
        without a grammar).
        sampling: a SamplingParams for every prompt, or one per prompt (all with one seed).  Token j of prompt b is then
        drawn by ops.sample with step = j and stream = streams[b] (default b), the first on the logits prefill / extend
        return and the later ones on step's; a temperature of 0 gives the greedy token.  Under a grammar the draw is
        among the tokens the state allows: grammar_argmax hands out their bits (its own token is dropped and the state
        it moved is discarded), sample draws under the bits, grammar_advance moves the state behind the drawn token.
        None: greedy, the code path without sampling.
        speculate: k in 0..7 -- up to k drafted tokens per sequence are verified in one forward (_speculative_loop); the
        ids returned are those of speculate=0 whatever is drafted.  drafter: (ids, max_draft) -> ids, default
        speculate.propose_drafts.  last_speculation then holds the forwards and the drafted / accepted counts per
        prompt (None with 0, which runs the plain loop).
        logprobs: None launches nothing.  n in 0..16: every produced token is scored by ops.logprobs on the logits it was
        picked from, the picked id still on the device -- in every picking mode and in both loops; under speculation a
        token is scored on the row that verified it, and a rejected draft leaves nothing.  last_logprobs[b] then holds one
        TokenLogprob (token, logprob, rank, allowed_logmass under a grammar, the n most likely (id, logprob)) per id
        returned for prompt b; a stop token leaves none.  The ids returned do not depend on it.
        penalties: a penalties.PenaltyParams for every prompt, or one per prompt (1..max_seqs prompts).  Every pick then
        first runs ops.adjust_logits -- the rule is penalties.adjust_host -- over the sequence's prompt and the ids
        picked so far, which the picker logs on the device, and picks on the adjusted rows: greedy takes the kernel's
        token, sampling and the grammar read the adjusted rows; while fewer than min_new_tokens ids are out, stop_ids are
        biased to -inf.  penalty_exempt: ids no penalty touches (penalties.exempt_ids).  logprobs keeps scoring the raw
        logits, and speculate=k returns the ids of speculate=0.  None or a neutral value: nothing is allocated or
        launched, the code path without penalties."""
        max_new_tokens, speculate = int(max_new_tokens), self._check_speculate(speculate)
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be positive")
        room = self.max_context - max_new_tokens
        longest = max(len(p) for p in prompts)
        if longest > room:
            raise PromptTooLong(f"a prompt of {longest} tokens does not fit: max_context {self.max_context} - "
                                f"max_new_tokens {max_new_tokens} leaves {room}")
        stop = {int(s) for s in stop_ids}
        pick = _Picker(self, len(prompts), grammar, sampling, streams, logprobs, penalties, prompts, max_new_tokens, stop,
                       penalty_exempt)
        keeps = [0] * len(prompts)
        if reuse_prefix and len(prompts) <= self.max_seqs:
            keeps = [plan_reuse(self.resident(b), p, PREFIX_MIN_REUSE) for b, p in enumerate(prompts)]
        if any(keeps):
            for b, keep in enumerate(keeps):
                self.truncate(b, keep)
            logits = self.extend([list(p[keep:]) for p, keep in zip(prompts, keeps)])
        else:
            logits = self.prefill(prompts)
        self.last_reuse = {"reused": list(keeps), "computed": [len(p) - keep for p, keep in zip(prompts, keeps)]} \
            if reuse_prefix else None
        out, accepted = self._decode(pick, [list(p) for p in prompts], logits, self.last_tokens, max_new_tokens, stop,
                                     speculate, drafter)
        self.last_grammar = {"accepted": accepted} if grammar is not None else None
        self.last_logprobs = pick.records
        return out

    @staticmethod
    def _check_speculate(speculate: int) -> int:
        if not 0 <= int(speculate) <= MAX_SPECULATE:
            raise ValueError(f"speculate must be in 0..{MAX_SPECULATE}")
        return int(speculate)

    def _decode(self, pick: _Picker, prompts: List[List[int]], logits, greedy, max_new_tokens: int, stop: set,
                speculate: int, drafter) -> Tuple[List[List[int]], List[bool]]:
        """The token loop of generate and generate_samples: the plain one, or the speculative one under speculate > 0."""
        self.last_speculation = None
        if speculate == 0:
            return self._token_loop(pick, len(prompts), logits, greedy, max_new_tokens, stop)
        return self._speculative_loop(pick, prompts, logits, greedy, max_new_tokens, stop, speculate,
                                      drafter or propose_drafts)

    def _token_loop(self, pick: _Picker, n: int, logits: torch.Tensor, greedy: torch.Tensor, max_new_tokens: int,
                    stop: set) -> Tuple[List[List[int]], List[bool]]:
        """The steps of generate and generate_samples behind the prompt: sequence b sits in slot b, `logits` / `greedy`
        [n] are what the prompt's last rows gave.  Returns (the new ids per sequence, whether each ended on a stop token
        of the grammar's table)."""
        out: List[List[int]] = [[] for _ in range(n)]
        live = list(range(n))
        accepted = [False] * n
        produced = 0    # tokens every live sequence has so far, the step of the next draw
        while live:
            feed, keep = [], []
            for k, (b, tok) in enumerate(zip(live, pick(live, logits, greedy, produced))):
                if pick.table is not None and tok >= 0 and pick.table.kind[tok] == KIND_STOP:
                    accepted[b] = True
                    continue
                if tok in stop or tok < 0:
                    continue
                out[b].append(int(tok))
                pick.file(b, k)
                if len(out[b]) < max_new_tokens:
                    keep.append(b)
                    feed.append(int(tok))
            live = keep
            if live:
                self.live = list(live)
                greedy, logits = self.step(feed)
                produced += 1
        self.live = []
        return out, accepted

    def _speculative_loop(self, pick: _Picker, prompts: List[List[int]], logits: torch.Tensor, greedy: torch.Tensor,
                          max_new_tokens: int, stop: set, speculate: int, drafter
                          ) -> Tuple[List[List[int]], List[bool]]:
        """_token_loop with drafts.  Sequence b (slot b, prompt prompts[b]) with the pending token t gets up to D_b =
        min(speculate, MAX_ROWS // live - 1, tokens still allowed - 1, context room) drafts d1..dm from drafter(prompt +
        output, D_b) -- the output ends in t -- and one step_rows feeds [t, d1..dm]; row i's logits are the logits behind
        t, d1..di.  The rows of a sequence are then picked in order through `pick`, each with the sequence's own count
        of produced tokens as the draw's step, and every pick is emitted exactly as _token_loop emits it; picking goes
        on to row i + 1 only when pick i equals draft i + 1, so a token is only ever picked on logits computed behind
        the tokens actually emitted, and the grammar state moves behind emitted tokens only.  The slot is cut back to
        the rows of t and the accepted drafts (truncate).  If nobody has a draft the iteration is a plain step."""
        n = len(prompts)
        out: List[List[int]] = [[] for _ in range(n)]
        accepted = [False] * n
        produced = [0] * n           # tokens picked per sequence: the step of its next draw
        stats = {"forwards": 0, "drafted": [0] * n, "accepted": [0] * n}
        pending = {b: (logits[b:b + 1], greedy[b:b + 1], [], 0) for b in range(n)}   # rows, greedy, drafts, cache length before
        live = list(range(n))
        while live:
            feed, keep = [], []
            for b in live:
                rows, tokens, drafts, base = pending[b]
                right, alive = 0, False
                for i in range(rows.shape[0]):
                    tok = pick([b], rows[i:i + 1], tokens[i:i + 1], produced[b])[0]
                    produced[b] += 1
                    if pick.table is not None and tok >= 0 and pick.table.kind[tok] == KIND_STOP:
                        accepted[b] = True
                        break
                    if tok in stop or tok < 0:
                        break
                    out[b].append(int(tok))
                    pick.file(b, 0)   # scored on row i, the row that verified it; a rejected draft is never picked
                    if len(out[b]) >= max_new_tokens:
                        break
                    if i < len(drafts) and drafts[i] == tok:   # row i + 1 was computed behind the right token
                        right += 1
                        continue
                    alive = True
                    break
                if drafts:
                    self.truncate(b, base + 1 + right)
                    stats["accepted"][b] += right
                if alive:
                    keep.append(b)
                    feed.append(out[b][-1])
            live = keep
            if not live:
                break
            self.live = list(live)
            token_rows = []
            for b, tok in zip(live, feed):
                room = min(speculate, MAX_ROWS // len(live) - 1, max_new_tokens - len(out[b]) - 1,
                           self.max_context - self.cache.lens[b] - 1)
                drafts = [int(d) for d in drafter(prompts[b] + out[b], room)][:room] if room > 0 else []
                bad = [i for i, d in enumerate(drafts) if not 0 <= d < self.cfg.vocab_size]
                token_rows.append([tok] + (drafts[:bad[0]] if bad else drafts))
            stats["forwards"] += 1
            if all(len(row) == 1 for row in token_rows):
                greedy, logits = self.step(feed)
            else:
                bases = [self.cache.lens[b] for b in live]
                greedy, logits = self.step_rows(token_rows)
            lo = 0
            for k, (b, row) in enumerate(zip(live, token_rows)):
                hi = lo + len(row)
                pending[b] = (logits[lo:hi], greedy[lo:hi], row[1:], bases[k] if len(row) > 1 else 0)
                stats["drafted"][b] += len(row) - 1
                lo = hi
        self.live = []
        self.last_speculation = stats
        return out, accepted

    @torch.no_grad()
    def score(self, prompts: Sequence[Sequence[int]], continuations: Sequence[Sequence[int]],
              slots: Optional[Sequence[int]] = None, top: int = 0, keep_logits: bool = False
              ) -> List[List[TokenLogprob]]:
        """Teacher-forced records of given continuations: for each of the 1..max_seqs sequences one TokenLogprob per id
        of continuations[b], scored behind prompts[b] and the ids before it, with the `top` (0..16) most likely ids of
        its row -- generate(logprobs=top)'s records for text the generator is handed.  prefill's layers run over prompt +
        continuation (PromptTooLong as from prefill); crag_enc_lm_head and crag_enc_logprobs then run over the rows that
        predict a continuation id in blocks of at most 8, so [rows, vocab] never exists beyond one block.  Afterwards
        slot slots[b] (default b) holds prompt + continuation as after a prefill, ids and all, for a following
        generate(reuse_prefix=True).  keep_logits (tests with tiny vocabularies): last_score_logits[b] keeps the fp32
        logits [len(continuations[b]), vocab] that were scored; None otherwise."""
        n = len(prompts)
        slots = self._check_slots("score takes 1..%d sequences, each in a slot of its own", n, slots)
        top = _check_logprobs(top, self.cfg.vocab_size)
        if len(continuations) != n or any(len(p) < 1 for p in prompts) or any(len(c) < 1 for c in continuations):
            raise ValueError("score needs one continuation per prompt, and at least one token in each of them")
        conts = [[int(t) for t in c] for c in continuations]
        full = [[int(t) for t in p] + c for p, c in zip(prompts, conts)]
        resid, delta, _ = self._prefill_rows(full, slots)
        # packed row start + len(prompt) - 1 + j predicts continuation id j
        rows, ids, start = [], [], 0
        for p, c, seq in zip(prompts, conts, full):
            rows += [start + len(p) - 1 + j for j in range(len(c))]
            ids += c
            start += len(seq)
        records: List[TokenLogprob] = []
        kept: List[torch.Tensor] = []
        for lo in range(0, len(rows), MAX_ROWS):
            idx = torch.tensor(rows[lo:lo + MAX_ROWS], dtype=torch.int64).to(self.device)
            logits, _ = self._head(resid.index_select(0, idx), delta.index_select(0, idx))
            token = torch.tensor(ids[lo:lo + MAX_ROWS], dtype=torch.int32).to(self.device)
            records += score_rows(logits, token, top)
            if keep_logits:
                kept.append(logits)
        out, logit_rows, lo = [], [], 0
        every = torch.cat(kept) if keep_logits else None
        for c in conts:
            out.append(records[lo:lo + len(c)])
            if keep_logits:
                logit_rows.append(every[lo:lo + len(c)])
            lo += len(c)
        self.last_score_logits = logit_rows if keep_logits else None
        return out

    def fork(self, src: int, dst_slots: Sequence[int]) -> None:
        """KvCache.fork: the dst slots hold what src holds without a copy.  Their ids count as unknown, so plan_reuse
        never keeps a child's rows."""
        self.cache.fork(src, dst_slots)
        for d in dst_slots:
            self.tokens[int(d)] = [-1] * self.cache.lens[int(d)]

    @torch.no_grad()
    def generate_samples(self, prompt: Sequence[int], n: int, max_new_tokens: int, stop_ids: Sequence[int] = (),
                         reuse_prefix: bool = False, grammar: Optional[TokenGrammar] = None,
                         sampling=None, streams: Optional[Sequence[int]] = None, speculate: int = 0,
                         drafter=None, logprobs: Optional[int] = None, penalties: Optional[PenaltyParams] = None,
                         penalty_exempt: Optional[Sequence[int]] = None) -> List[List[int]]:
        """n (1..max_seqs) continuations of ONE prompt from one prefill: the prompt goes into slot 0 (prefill, or extend
        behind what plan_reuse keeps under reuse_prefix, as in generate), slots 1..n-1 are forked from it, the one row
        of logits serves every sequence's first pick, and generate's token loop runs over the n slots: a child reads
        the prompt's rows in the parent's slot (crag_enc_decode_attention_shared) and appends to its own.  Sequence i
        draws on streams[i] (default i).  A sequence that stops -- slot 0 too -- leaves the others running on its rows.
        Afterwards the children are empty and slot 0 holds the prompt and continuation 0 with their ids, for a later
        reuse_prefix.  last_reuse / last_grammar hold one entry per sample (the prompt's rows were reused / computed
        once, for all of them).  n = 1 is generate([prompt], ...).  speculate / drafter: as in generate; every sample
        drafts from the prompt and its own output.  logprobs: as in generate, last_logprobs[i] for sample i.  penalties /
        penalty_exempt: as in generate, one value for every sample; each sample is penalised for its own output."""
        n, max_new_tokens, speculate = int(n), int(max_new_tokens), self._check_speculate(speculate)
        if not 1 <= n <= self.max_seqs:
            raise ValueError(f"generate_samples takes n in 1..{self.max_seqs}")
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be positive")
        room = self.max_context - max_new_tokens
        if len(prompt) > room:
            raise PromptTooLong(f"a prompt of {len(prompt)} tokens does not fit: max_context {self.max_context} - "
                                f"max_new_tokens {max_new_tokens} leaves {room}")
        if penalties is not None and not isinstance(penalties, PenaltyParams):
            raise ValueError("generate_samples takes one PenaltyParams for all samples")
        pick = _Picker(self, n, grammar, sampling, streams, logprobs, penalties, [prompt] * n, max_new_tokens,
                       {int(s) for s in stop_ids}, penalty_exempt)
        keep = plan_reuse(self.resident(0), prompt, PREFIX_MIN_REUSE) if reuse_prefix else 0
        if keep:
            self.truncate(0, keep)
            logits = self.extend([list(prompt[keep:])])
        else:
            logits = self.prefill([prompt])
        self.last_reuse = {"reused": [keep] * n, "computed": [len(prompt) - keep] * n} if reuse_prefix else None
        greedy = self.last_tokens
        try:
            if n > 1:
                self.fork(0, range(1, n))
                logits, greedy = logits.repeat(n, 1), greedy.repeat(n)
            out, accepted = self._decode(pick, [list(prompt)] * n, logits, greedy, max_new_tokens,
                                         {int(s) for s in stop_ids}, speculate, drafter)
        finally:
            self.live = []
            for child in range(1, n):
                self.truncate(child, 0)
        self.last_grammar = {"accepted": accepted} if grammar is not None else None
        self.last_logprobs = pick.records
        return out

    def generate_text_samples(self, messages: Sequence[Dict[str, str]], n: int, max_new_tokens: int,
                              grammar: Optional[TokenGrammar] = None, sampling: Optional[SamplingParams] = None,
                              streams: Optional[Sequence[int]] = None, speculate: int = 0, drafter=None,
                              logprobs: Optional[int] = None, penalties: Optional[PenaltyParams] = None,
                              penalty_exempt: Optional[Sequence[int]] = None) -> List[str]:
        """One chat -> n replies as text from one prefill (generate_samples), reply i drawn on noise stream streams[i];
        logprobs: last_logprobs[i] holds reply i's records; penalties / penalty_exempt: as in generate."""
        ids = self.generate_samples(self.chat_ids(messages), n, max_new_tokens, self.stop_ids(),
                                    reuse_prefix=self.prefix_cache, grammar=grammar, sampling=sampling, streams=streams,
                                    speculate=speculate, drafter=drafter, logprobs=logprobs, penalties=penalties,
                                    penalty_exempt=penalty_exempt)
        tok = self._tokenizer()
        return [tok.decode(x, skip_special_tokens=True) for x in ids]

    def generate_text(self, messages: Sequence[Dict[str, str]], max_new_tokens: int,
                      grammar: Optional[TokenGrammar] = None, sampling: Optional[SamplingParams] = None,
                      stream: int = 0, speculate: int = 0, drafter=None, logprobs: Optional[int] = None,
                      penalties: Optional[PenaltyParams] = None, penalty_exempt: Optional[Sequence[int]] = None) -> str:
        """One chat -> the assistant's reply as text; under `grammar` when one is given, drawn with `sampling` on noise
        stream `stream` when that is given (generate); logprobs: last_logprobs[0] holds the reply's records; penalties /
        penalty_exempt: as in generate."""
        ids = self.generate([self.chat_ids(messages)], max_new_tokens, self.stop_ids(),
                            reuse_prefix=self.prefix_cache, grammar=grammar, sampling=sampling,
                            streams=None if sampling is None else [int(stream)], speculate=speculate,
                            drafter=drafter, logprobs=logprobs, penalties=penalties, penalty_exempt=penalty_exempt)[0]
        return self._tokenizer().decode(ids, skip_special_tokens=True)
