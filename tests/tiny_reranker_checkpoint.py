"""Builds a tiny LOCAL Qwen3-Reranker-shaped checkpoint directory (config.json, model.safetensors, tokenizer files) so
that Qwen3Reranker.from_pretrained runs in tests without any download.

Everything is this repository's own data: a byte-level BPE tokenizer trained here on the sentences below (the chat
markers as special tokens, "yes" and "no" single tokens, as in the Qwen3 vocabulary) and a seeded random 2-layer
Qwen3ForCausalLM written with bf16-representable weights, lm_head included.  Two variants: an untied lm_head (the 4B
model) and one tied to embed_tokens (the 0.6B model).
"""
from __future__ import annotations

from pathlib import Path

import torch

EOS = "<|endoftext|>"
SPECIALS = [EOS, "<|im_start|>", "<|im_end|>"]
CORPUS = [
    "the customer called about a failed deployment of the api gateway",
    "we saw ECONNRESET errors between the gateway and the billing service after the upgrade",
    "ticket ABC-123 tracks the rollback to version v1.2.3 and the follow up call next week",
    "the agent confirmed the refund and scheduled a call back for tuesday morning",
    "latency went from forty milliseconds to nine hundred during the incident window",
    "numbers 0 1 2 3 4 5 6 7 8 9 and punctuation , . ; : ! ? ( ) [ ] { } - _ / \\ ' \"",
    "Judge whether the Document meets the requirements based on the Query and the Instruct provided.",
    "Note that the answer can only be \"yes\" or \"no\".",
    "<Instruct>: Given a web search query, retrieve relevant passages that answer the query",
    "<Query>: <Document>: system user assistant <think> </think>",
]
YES_NO = ["yes", "no", "\"yes\"", "\"no\"", "yes.", "no."]


def build_tokenizer(vocab_size: int = 448):
    """Byte-level BPE, no post-processor (the Qwen3 tokenizer adds no special tokens to a plain call)."""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, trainers
    from transformers import PreTrainedTokenizerFast
    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(vocab_size=vocab_size, special_tokens=SPECIALS,
                                  initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False)
    tok.train_from_iterator(CORPUS * 4 + YES_NO * 64, trainer)
    out = PreTrainedTokenizerFast(tokenizer_object=tok, eos_token=EOS, pad_token=EOS,
                                  additional_special_tokens=SPECIALS[1:])
    for w in ("yes", "no"):
        assert out.encode(w, add_special_tokens=False) == [out.get_vocab()[w]], f"{w!r} is not a single token"
    return out


def build_checkpoint(root, *, tied: bool = False, layers: int = 2, seed: int = 5151, heads=(4, 2)):
    """Writes the directory and returns (hf Qwen3ForCausalLM fp32 on the CPU with bf16-representable weights,
    tokenizer)."""
    from safetensors.torch import save_file
    from transformers import Qwen3Config as HFConfig
    from transformers import Qwen3ForCausalLM
    root = Path(root)
    root.mkdir(parents=True, exist_ok=True)
    tokenizer = build_tokenizer()
    tokenizer.save_pretrained(str(root))
    torch.manual_seed(seed)
    cfg = HFConfig(vocab_size=len(tokenizer), hidden_size=256, intermediate_size=512, num_hidden_layers=layers,
                   num_attention_heads=heads[0], num_key_value_heads=heads[1], head_dim=128, rms_norm_eps=1e-6,
                   max_position_embeddings=2048, rope_parameters={"rope_theta": 1_000_000.0, "rope_type": "default"},
                   attention_bias=False, tie_word_embeddings=tied)
    model = Qwen3ForCausalLM(cfg).eval()
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(1 + 0.1 * torch.randn_like(p) if "norm" in name else torch.randn_like(p) * 0.05)
            p.copy_(p.to(torch.bfloat16).float())
    cfg.save_pretrained(str(root))
    sd = {k: v.to(torch.bfloat16).contiguous() for k, v in model.state_dict().items()}
    if tied:
        sd.pop("lm_head.weight", None)
    save_file(sd, str(root / "model.safetensors"))
    return model, tokenizer
