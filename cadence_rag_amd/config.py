"""Settings for the dense lane — the EMBEDDINGS_* knobs of the reference
(/root/reference/app/config.py:10-16,25-26) with the same names, defaults and env-var spelling
(case-insensitive, no prefix).  Plain dataclass: the reference's pydantic-settings object is
mutated by its tests with monkeypatch.setattr(settings, ...), and so is this one.

The RERANK_* knobs are the reference's Phase-4 plan (PHASED_PLAN.md:291-297), same names and spelling; the LLM_* knobs
its Phase-5 plan (PHASED_PLAN.md:318-326).

New knob: EMBEDDINGS_BASE_URL keeps its meaning ("" disables the dense lane); the value
"native" (or "native://...") selects the in-process MI355X encoder instead of an HTTP gateway.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, fields


def _env(name: str, default):
    for key, raw in os.environ.items():
        if key.lower() == name.lower():
            if isinstance(default, bool):
                return raw.strip().lower() in ("1", "true", "yes", "on")
            return type(default)(raw)
    return default


@dataclass
class Settings:
    embeddings_base_url: str = ""
    embeddings_model_id: str = "Qwen/Qwen3-Embedding-4B"
    embeddings_dim: int = 1024
    embeddings_timeout_s: float = 180.0
    embeddings_batch_size: int = 32
    embeddings_exact_scan_threshold: int = 2000
    embeddings_hnsw_ef_search: int = 80
    ingest_auto_embed_on_success: bool = True
    ingest_auto_embed_fail_on_error: bool = False
    # native lane only
    embeddings_device: int = 0
    embeddings_max_length: int = 1024  # gateway truncation (RUNBOOK:484,748)
    # reranker (PHASED_PLAN.md:291-297): "" = off, "native" = the in-process Qwen3Reranker, http(s) = a /rerank service
    rerank_base_url: str = ""
    rerank_model_id: str = "Qwen/Qwen3-Reranker-4B"
    rerank_timeout_s: float = 180.0
    rerank_max_chars_per_doc: int = 0   # 0: no character cut (the model truncates to rerank_max_length tokens)
    rerank_topn_in: int = 40            # fused rows scored per side
    rerank_topm_out: int = 12           # rows kept per side after reranking
    rerank_max_length: int = 1024
    rerank_device: int = -1             # -1: embeddings_device
    # near-duplicate suppression of each side's fused list, in front of the reranker (the reference's planned "dedupe
    # rules", PHASED_PLAN.md:299-303): a fused row is dropped when a kept, higher-ranked row of its side has at least
    # this cosine with it.  0.0 = off
    evidence_dedupe_cosine: float = 0.0
    # per-call cap of the chunk dense lane (the reference's planned "per-call diversity caps", PHASED_PLAN.md:299-303):
    # at most this many chunks of one call among the lane's rows, applied over the whole table (the grouped search), so
    # that one long call cannot fill the lane while _pack keeps DEFAULT_MAX_QUOTES_PER_CALL of it.  0 = off
    dense_per_call_cap: int = 0
    # maximal marginal relevance on the dense lanes (the graded form of the reference's planned redundancy control,
    # PHASED_PLAN.md:286-303): the lane fetches dense_mmr_fetch rows (0: min(4 x its limit, 256); a search returns at most
    # CRAG_MAX_K) and picks its limit among them by lambda * cosine to the query - (1 - lambda) * the largest cosine to a
    # row picked before (crag_index_mmr_async).  1.0 = the plain ranking = off: nothing is launched
    dense_mmr_lambda: float = 1.0
    dense_mmr_fetch: int = 0
    # clause syntax of the BM25 word lane (cadence_rag_amd.bm25.parse_query: +required, -excluded, "quoted phrase"; a
    # self-defined rule, not Tantivy's parser).  Phrases need lanes built with positions (build_bm25_lane(...,
    # positions=True)).  Off: the query string is a bag of tokens and nothing is launched
    bm25_query_syntax: bool = False
    # prefix and fuzzy items of that syntax (`deploy*`, `kubernets~`, `kubernets~2`: parse_query(text, expand=True),
    # DESIGN.md 4.7d): the word lane expands them over its vocabulary on the GPU, one stream synchronisation per query that
    # holds one.  Takes effect only together with bm25_query_syntax.  Off: `*` and `~` separate tokens as ever
    bm25_query_expand: bool = False
    # query-aware snippets of /retrieve (env RETRIEVE_SNIPPET_BEST, RETRIEVE_SNIPPET_WINDOW_TOKENS): an
    # evidence item's snippet is cut around the window of snippet_window_tokens tokens that holds the most of the query,
    # found by the word lane on the GPU (it must be built with positions), instead of the first 800 characters.  Off:
    # nothing is asked, nothing is launched and every response is what it was
    snippet_best: bool = False
    snippet_window_tokens: int = 120
    # /answer (PHASED_PLAN.md:318-326): "" = off, "native" = the in-process Qwen3Generator, http(s) = an OpenAI-compatible
    # chat-completions service
    llm_base_url: str = ""
    llm_api_key: str = ""
    llm_model: str = "Qwen/Qwen3-4B-Instruct-2507"
    llm_timeout_s: float = 180.0
    llm_max_new_tokens: int = 512
    llm_max_context: int = 8192
    llm_device: int = -1                # -1: embeddings_device
    llm_prefix_cache: bool = True       # native LLM: a prompt that continues what its slot holds computes only the rest
    answer_max_repairs: int = 2         # reprompts of an answer that fails the citation check
    # native LLM only: decode under the citation grammar of the evidence in the prompt (cadence_rag_amd.grammar), so that
    # an uncited sentence or an id outside the pack cannot be generated; the validator still checks what comes back
    answer_constrained: bool = False
    # sampling defaults of /answer (cadence_rag_amd.sampling); a request's own temperature / top_p / top_k / min_p / seed
    # override them.  Temperature 0 is greedy decoding: with these defaults /answer is what it was without sampling
    answer_temperature: float = 0.0
    answer_top_p: float = 1.0
    answer_top_k: int = 0
    answer_min_p: float = 0.0
    answer_seed: int = 0
    # candidates drawn per attempt (1..8; a request's `samples` overrides it).  Above 1 -- sampling on, a native model with
    # generate_text_samples -- one prefill serves all of them and the first that passes the citation check is the answer
    answer_samples: int = 1
    # speculative decoding of /answer (0..7; a request's `speculate` overrides it): a native model with
    # supports_speculation verifies up to that many prompt-lookup drafts per forward.  The reply does not depend on it;
    # 0 = off, the plain token loop
    answer_speculate: int = 0
    # token log-probabilities of /answer (a request's `logprobs` overrides it): a native model with supports_logprobs
    # scores every token it produces (crag_enc_logprobs) and notes.logprobs describes the returned answer.  Off: nothing
    # is launched and there is no such note
    answer_logprobs: bool = False
    # how the answer is chosen among several valid candidates (a request's `sample_rank` overrides it): "first" -- the
    # lowest index -- or "logprob" -- the highest mean token log-probability, which needs samples > 1 and such a model
    answer_sample_rank: str = "first"
    # repetition control of /answer (cadence_rag_amd.penalties); a request's own field of the same name overrides each.
    # All neutral by default: nothing is launched and the response is what it was.  ANSWER_LOGIT_BIAS is a JSON object
    # as text, token id -> value ('{"1234": -100}'; "" is none).  A native model with supports_penalties applies all of
    # them on the GPU (crag_enc_adjust_logits); an HTTP service gets presence_penalty, frequency_penalty and logit_bias
    answer_repetition_penalty: float = 1.0
    answer_presence_penalty: float = 0.0
    answer_frequency_penalty: float = 0.0
    answer_no_repeat_ngram: int = 0
    answer_logit_bias: str = ""
    answer_min_new_tokens: int = 0

    def __post_init__(self) -> None:
        if self.rerank_device < 0:
            self.rerank_device = self.embeddings_device
        if self.llm_device < 0:
            self.llm_device = self.embeddings_device

    @classmethod
    def from_env(cls) -> "Settings":
        return cls(**{f.name: _env(_ENV_NAMES.get(f.name, f.name), f.default) for f in fields(cls)})


# knobs whose environment variable is not the field's own name
_ENV_NAMES = {"snippet_best": "RETRIEVE_SNIPPET_BEST", "snippet_window_tokens": "RETRIEVE_SNIPPET_WINDOW_TOKENS"}


settings = Settings.from_env()
