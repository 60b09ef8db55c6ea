"""Qwen3-Reranker on MI355X: the Qwen3-Embedding decoder (Qwen3Encoder) with the reranker's prompt and head.

A pair is scored as the model card does it: the prompt template below around "<Instruct>: ... <Query>: ...
<Document>: ...", one causal forward, the final norm of the LAST token, the "yes" and "no" rows of lm_head, and
score = exp(log_softmax([no, yes])[1]).

What the card's padded batch recomputes for every pair is shared here: the pairs of one call begin with the same
token ids (system prompt, instruction, query), so a forward packs that common id prefix ONCE as a root segment and
every pair as a child segment that attends to it (PackedBatch.build_prefixed, crag_enc_attention_prefixed).  The
prefix is found on token ids, never on text, so sharing cannot change a pair's ids: prefix + child == the card's ids.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .qwen3 import PackedBatch, Qwen3Config, Qwen3Encoder

# the Qwen3-Reranker model card's template, verbatim
PREFIX = ("<|im_start|>system\nJudge whether the Document meets the requirements based on the Query and the Instruct "
          "provided. Note that the answer can only be \"yes\" or \"no\".<|im_end|>\n<|im_start|>user\n")
SUFFIX = "<|im_end|>\n<|im_start|>assistant\n<think>\n\n</think>\n\n"
PAIR = "<Instruct>: {instruction}\n<Query>: {query}\n<Document>: {doc}"
DEFAULT_INSTRUCTION = "Given a web search query, retrieve relevant passages that answer the query"
DEFAULT_TOKEN_BUDGET = 65536


def canonical_ids(tokenizer, query: str, documents: Sequence[str], instruction: str, max_length: int
                  ) -> List[List[int]]:
    """The model card's ids of every (query, document) pair: prefix + pair (truncated, longest_first: the document's
    tail goes) + suffix, at most max_length tokens."""
    prefix_ids = tokenizer.encode(PREFIX, add_special_tokens=False)
    suffix_ids = tokenizer.encode(SUFFIX, add_special_tokens=False)
    room = int(max_length) - len(prefix_ids) - len(suffix_ids)
    if room <= 0:
        raise ValueError(f"max_length {max_length} leaves no room for a pair beside the prompt template")
    pairs = [PAIR.format(instruction=instruction, query=query, doc=d) for d in documents]
    body = tokenizer(pairs, padding=False, truncation="longest_first", return_attention_mask=False,
                     max_length=room)["input_ids"]
    return [list(prefix_ids) + list(b) + list(suffix_ids) for b in body]


def shared_prefix_len(token_lists: Sequence[Sequence[int]]) -> int:
    """Longest common id prefix of the lists, capped so that every list keeps at least one token of its own."""
    if not token_lists:
        return 0
    cap = min(len(tl) for tl in token_lists) - 1
    first = token_lists[0]
    n = 0
    while n < cap and all(tl[n] == first[n] for tl in token_lists):
        n += 1
    return n


def split_forwards(lengths: Sequence[int], prefix_len: int, budget: int) -> List[List[int]]:
    """Pair indices per forward, in order: each forward holds its own copy of the prefix (prefix_len tokens) plus
    the pairs' own tokens (lengths[i] - prefix_len) within `budget` tokens; a pair that alone exceeds it goes alone."""
    groups: List[List[int]] = []
    cur: List[int] = []
    used = prefix_len
    for i, n in enumerate(lengths):
        own = int(n) - prefix_len
        if cur and used + own > budget:
            groups.append(cur)
            cur, used = [], prefix_len
        cur.append(i)
        used += own
    if cur:
        groups.append(cur)
    return groups


class Qwen3Reranker:
    """rerank(query, documents) -> (scores fp32 [n], order, model id) on one GPU."""

    def __init__(self, encoder: Qwen3Encoder, lm_rows: torch.Tensor, tokenizer=None, *,
                 instruction: Optional[str] = None, token_budget: int = DEFAULT_TOKEN_BUDGET,
                 model_id: Optional[str] = None) -> None:
        c = encoder.cfg
        if c.num_heads % c.num_kv_heads or c.num_heads // c.num_kv_heads not in (2, 4):
            raise ValueError("the prefix-aware attention kernel is built for 2 or 4 query heads per kv head")
        if tuple(lm_rows.shape) != (2, c.hidden_size):
            raise ValueError(f"lm_rows must be [2, {c.hidden_size}] (the 'yes' and 'no' rows of lm_head)")
        if int(token_budget) < 1:
            raise ValueError("token_budget must be positive")
        self.encoder = encoder
        self.head = lm_rows.to(device=encoder.device, dtype=torch.bfloat16).contiguous()
        self.tokenizer = tokenizer
        self.instruction = instruction or DEFAULT_INSTRUCTION
        self.token_budget = int(token_budget)
        self.model_id = model_id or c.model_id
        self.last_stats: Dict[str, int] = {}

    @property
    def max_length(self) -> int:
        return self.encoder.cfg.max_length

    @classmethod
    def from_pretrained(cls, path: str, device: Optional[torch.device] = None, max_length: int = 1024,
                        instruction: Optional[str] = None, *, token_budget: int = DEFAULT_TOKEN_BUDGET,
                        model_id: Optional[str] = None) -> "Qwen3Reranker":
        """A local *ForCausalLM checkpoint directory (config.json, *.safetensors, tokenizer files; nothing is fetched).
        Only the "yes" and "no" rows of lm_head are kept on the device (from embed_tokens when the checkpoint ties
        them)."""
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
                          max_length=int(max_length), out_dim=min(1024, hf["hidden_size"]), pooling="last",
                          model_id=model_id or hf.get("_name_or_path") or str(root.name))
        tokenizer = AutoTokenizer.from_pretrained(str(root), local_files_only=True)
        yes_no = [cls._single_token_id(tokenizer, w) for w in ("yes", "no")]
        cls._check_template(tokenizer)
        files = sorted(root.glob("*.safetensors"))
        if not files:
            raise FileNotFoundError(f"no *.safetensors under {root}")
        sd: Dict[str, torch.Tensor] = {}
        for f in files:
            sd.update(load_file(str(f)))
        prefix = "model." if any(k.startswith("model.") for k in sd) else ""
        if hf.get("tie_word_embeddings", False) or "lm_head.weight" not in sd:
            if not hf.get("tie_word_embeddings", False):
                raise ValueError(f"{root}: no lm_head.weight and the config does not tie it to embed_tokens")
            table = sd[prefix + "embed_tokens.weight"]
        else:
            table = sd["lm_head.weight"]
        lm_rows = table[yes_no].to(torch.bfloat16).contiguous()
        sd.pop("lm_head.weight", None)
        enc = Qwen3Encoder.from_state_dict(cfg, sd, device, prefix=prefix)
        enc.tokenizer = tokenizer
        return cls(enc, lm_rows, tokenizer, instruction=instruction, token_budget=token_budget, model_id=cfg.model_id)

    @staticmethod
    def _single_token_id(tokenizer, word: str) -> int:
        vocab = tokenizer.get_vocab()
        if word not in vocab or tokenizer.encode(word, add_special_tokens=False) != [vocab[word]]:
            raise ValueError(f"the reranker needs {word!r} as a single vocabulary token; this tokenizer splits it")
        return int(vocab[word])

    @staticmethod
    def _check_template(tokenizer) -> None:
        """The template's chat markers must be single tokens wherever the vocabulary has them (a Qwen3 tokenizer does):
        otherwise the checkpoint's prompt format is not the one this class writes."""
        vocab = tokenizer.get_vocab()
        for marker in ("<|im_start|>", "<|im_end|>"):
            if marker in vocab and tokenizer.encode(marker, add_special_tokens=False) != [vocab[marker]]:
                raise ValueError(f"{marker!r} is in the vocabulary but is not encoded as one token")

    # -- tokens ---------------------------------------------------------------------------------------------------
    def token_lists(self, query: str, documents: Sequence[str], instruction: Optional[str] = None) -> List[List[int]]:
        if self.tokenizer is None:
            raise RuntimeError("no tokenizer loaded (Qwen3Reranker.from_pretrained, or pass one)")
        return canonical_ids(self.tokenizer, query, documents, instruction or self.instruction, self.max_length)

    def plan(self, token_lists: Sequence[Sequence[int]], share_prefix: bool = True) -> Tuple[int, List[List[int]]]:
        """(shared prefix length, pair indices of every forward)."""
        p = shared_prefix_len(token_lists) if share_prefix else 0
        return p, split_forwards([len(tl) for tl in token_lists], p, self.token_budget)

    # -- forward --------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def score_token_lists(self, token_lists: Sequence[Sequence[int]], share_prefix: bool = True) -> np.ndarray:
        """[n, 3] fp32 = (logit_yes, logit_no, score) of every id list."""
        if not token_lists or any(len(tl) == 0 for tl in token_lists):
            raise ValueError("every pair needs at least one token")
        if max(len(tl) for tl in token_lists) > self.max_length:
            raise ValueError(f"a pair is longer than max_length {self.max_length}")
        p, groups = self.plan(token_lists, share_prefix)
        dev = self.encoder.device
        out = np.empty((len(token_lists), 3), dtype=np.float32)
        executed = 0
        for g in groups:
            if p > 0:
                lengths = [p] + [len(token_lists[i]) - p for i in g]
                parent = [-1] + [0] * len(g)
                flat = np.concatenate([np.asarray(token_lists[g[0]][:p], dtype=np.int32)]
                                      + [np.asarray(token_lists[i][p:], dtype=np.int32) for i in g])
            else:
                lengths = [len(token_lists[i]) for i in g]
                parent = [-1] * len(g)
                flat = np.concatenate([np.asarray(token_lists[i], dtype=np.int32) for i in g])
            batch = PackedBatch.build_prefixed(lengths, parent, dev)
            ids = torch.from_numpy(flat).to(dev)
            res = self.encoder.forward_packed(ids, batch, head=self.head)
            out[g] = res.cpu().numpy()
            executed += int(flat.size)
        self.last_stats = {"pairs": len(token_lists), "prefix_tokens": p, "forwards": len(groups),
                           "real_tokens": int(sum(len(tl) for tl in token_lists)), "executed_tokens": executed}
        return out

    def rerank(self, query: str, documents: Sequence[str], instruction: Optional[str] = None,
               share_prefix: bool = True) -> Tuple[np.ndarray, List[int], str]:
        """scores fp32 [n] (P("yes")), order = indices by descending score (ties: input order), model id."""
        if not documents:
            raise ValueError("rerank needs at least one document")
        scores = self.score_token_lists(self.token_lists(query, documents, instruction), share_prefix)[:, 2].copy()
        return scores, stable_order(scores), self.model_id


def stable_order(scores: Sequence[float]) -> List[int]:
    """Indices by descending score, ties resolved by index."""
    return sorted(range(len(scores)), key=lambda i: (-float(scores[i]), i))
