"""/answer: one-shot answering grounded strictly in the evidence pack, the reference's Phase 5 (PHASED_PLAN.md:312-340),
with reranker.py's client seam: AnswerClientError, set_llm, llm_enabled, validate_citations, answer_question.

LLM_BASE_URL="" turns answering off; "native" (or "native://...") routes to the in-process generator registered with
set_llm() (cadence_rag_amd.encoder.generate.Qwen3Generator); an http(s) URL speaks the OpenAI-compatible
`POST {base}/chat/completions`.  Every failure reaches the caller as AnswerClientError.

The gate: every sentence of an answer must cite at least one evidence id of the pack (`[Q-123]`, `[A-45]`, the
evidence_id format retrieve._pack emits).  An answer that fails is sent back with the validator's report at most
ANSWER_MAX_REPAIRS times; if it still fails, the response carries no answer.  No uncited sentence ever leaves.

Sampling (cadence_rag_amd.sampling): a request's temperature / top_p / top_k / min_p / seed, over the ANSWER_* defaults.
With a temperature of 0 and no such field in the request nothing changes: greedy decoding, the same HTTP body, the same
notes.  Otherwise a native model with supports_sampling draws every token on the GPU (crag_enc_sample), an HTTP service
gets temperature, top_p and seed, notes.sampling echoes the parameters, and repair round i draws on noise stream i.

Several candidates per attempt (`samples` of the request, ANSWER_SAMPLES; 1..8, sampling on): a native model with
supports_samples draws them from ONE prefill (Qwen3Generator.generate_text_samples: the candidates are forks of the
prompt's KV rows), attempt a on the noise streams a * n + i.  They are judged in index order: the first that passes the
gate is the answer; if every one is INSUFFICIENT_EVIDENCE so is the response; otherwise the first failing candidate that
is not INSUFFICIENT_EVIDENCE goes into the repair turn.  notes.samples = {"drawn", "valid", "chosen"} describes the last
attempt; llm_calls counts calls, not candidates.  An HTTP service, or a native model without supports_samples, gives one
candidate as ever and notes.samples = {"applied": False}.  With one sample nothing changes.

Speculative decoding (`speculate` of the request, ANSWER_SPECULATE; 0..7, off at 0): a native model with
supports_speculation verifies up to that many prompt-lookup drafts per forward (cadence_rag_amd.speculate); the reply
does not depend on it.  notes.speculation echoes the model's last_speculation; anything else decodes as ever and says
notes.speculation = {"applied": False}.  With 0 and no field the response and the notes are what they were.

Token log-probabilities (`logprobs` of the request, ANSWER_LOGPROBS; off by default): a native model with
supports_logprobs scores every token it produces on the GPU (crag_enc_logprobs: the model's own distribution at
temperature 1, whatever picked the token) and notes.logprobs = {"tokens", "mean_logprob", "min_logprob"} describes the
judged candidate, under the grammar also {"mean_allowed_logmass", "min_allowed_logmass"}: how much probability the
automaton left allowed, i.e. how hard it had to push.  Anything else says notes.logprobs = {"applied": False}.
`sample_rank` (ANSWER_SAMPLE_RANK): "first" judges candidates in index order as ever; "logprob" -- several candidates
from such a model -- takes the valid candidate with the highest mean token log-probability (the lowest index among
equals), ranks the candidate quoted into a repair turn the same way among those that tried to answer, and
notes.samples gains "scores" (one mean per candidate) and "ranked": True.  "logprob" with one sample, or on a backend
without the capability, behaves as "first" and says notes.samples["ranked"] = False.

Repetition control (cadence_rag_amd.penalties): a request's repetition_penalty / presence_penalty / frequency_penalty /
no_repeat_ngram / logit_bias / min_new_tokens, over the ANSWER_* defaults, all neutral.  A native model with
supports_penalties applies them on the GPU before every pick (crag_enc_adjust_logits), with the ids of the citation
alphabet "[]-0123456789QA" exempt, so that citing [Q-12] a second time is never penalised or banned; an HTTP service is
sent presence_penalty, frequency_penalty and logit_bias, and notes.penalties_ignored names the others that were set.
notes.penalties echoes the parameters (with "applied": False for a native model without the capability) only when
they are not neutral: a request that names none of this gets the response it always got.

ANSWER_CONSTRAINED (native backend, a model with supports_grammar): the reply is decoded under the citation grammar of
the evidence ids in the prompt (cadence_rag_amd.grammar.citation_grammar), which makes a failing answer unrepresentable
whenever the model stops by itself.  The gate and the repair loop run unchanged on whatever comes back.
"""
from __future__ import annotations

import re
import threading
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Protocol, Sequence, Tuple

from . import retrieve as _retrieve
from .config import settings
from .grammar import INSUFFICIENT as _INSUFFICIENT_BYTES
from .grammar import TokenGrammar, citation_grammar
from .logprobs import mean_logprob, summarise
from .penalties import CITATION_ALPHABET, PenaltyParams, active as _active_penalties, exempt_ids
from .sampling import SamplingParams

INSUFFICIENT = _INSUFFICIENT_BYTES.decode("ascii")   # "INSUFFICIENT_EVIDENCE": one definition, the grammar's
STATUS_OK = "ok"
STATUS_INSUFFICIENT = "insufficient_evidence"
STATUS_FAILED = "citation_check_failed"

SYSTEM_RULES = (
    "You answer questions about recorded calls. Use ONLY the evidence items listed by the user; never use outside "
    "knowledge. End every sentence with the id of each evidence item that supports it, in square brackets, exactly as "
    "given, for example [Q-123] or [A-45][Q-7]. A sentence without such an id is not allowed. If the evidence does not "
    "answer the question, reply with exactly " + INSUFFICIENT + " and nothing else.")


class AnswerClientError(RuntimeError):
    pass


class AnswerRequestError(ValueError):
    """The request itself is wrong (a sampling parameter out of range): nothing was retrieved or generated."""


class ChatModel(Protocol):
    """In-process backend: a chat (list of {"role", "content"}) -> the assistant's reply.  A ValueError means the prompt
    does not fit the context (the caller drops evidence and retries); any other exception is reported as
    AnswerClientError.  `model_id` names the model.
    Optional: a model whose class sets `supports_grammar = True` also takes `generate_text(messages, max_new_tokens,
    grammar=TokenGrammar)` and decodes only what grammar.dfa accepts; its `token_table()`, if it has one, is the cached
    byte table of its vocabulary that goes into the TokenGrammar.  The keyword is passed only to such a model.
    Optional: a model whose class sets `supports_sampling = True` also takes `sampling=SamplingParams, stream=int`.
    Optional: a model whose class sets `supports_samples = True` also has `generate_text_samples(messages, n,
    max_new_tokens, grammar=None, sampling=None, streams=None) -> List[str]`: n replies to one chat, reply i drawn on
    noise stream streams[i]; the same exceptions as generate_text.
    Optional: a model whose class sets `supports_logprobs = True` also takes `logprobs=int` in both and then leaves
    `last_logprobs`: per reply a list of cadence_rag_amd.logprobs.TokenLogprob, one per produced token.
    Optional: a model whose class sets `supports_penalties = True` also takes `penalties=PenaltyParams,
    penalty_exempt=ids or None` in both: repetition control, the exempt ids untouched by it."""

    model_id: str

    def generate_text(self, messages: Sequence[Dict[str, str]], max_new_tokens: int) -> str: ...


_llm: Optional[ChatModel] = None
_llm_lock = threading.Lock()  # one GPU submission at a time (FastAPI runs sync endpoints on a threadpool)


def set_llm(llm: Optional[ChatModel]) -> None:
    global _llm
    _llm = llm


def get_llm() -> Optional[ChatModel]:
    return _llm


def llm_enabled() -> bool:
    return bool(settings.llm_base_url.strip())


def _is_native(url: str) -> bool:
    return url.strip().lower().startswith("native")


# ---- the citation gate ------------------------------------------------------------------------------------------
_CITE = re.compile(r"\[(Q|A)-(\d+)\]")
# a sentence ends at . ! ? followed by whitespace or the end of the text; a citation group directly behind the
# terminator ("... text. [Q-12][A-45]") still belongs to that sentence
_SENTENCE_END = re.compile(r"[.!?]+(?:[ \t]*\[(?:Q|A)-\d+\])*(?=\s|$)")
_LIST_MARKER = re.compile(r"^\s*(?:[-*•]|\d+[.)])(?:\s+|$)")


def _normal_id(letter: str, digits: str) -> str:
    return f"{letter}-{int(digits)}"


def split_sentences(text: str) -> List[str]:
    """The sentences of an answer: per line (blank lines and bare list markers are none), cut behind . ! ? when
    whitespace or the end follows, a directly following citation group kept with the sentence before it."""
    out: List[str] = []
    for line in text.splitlines():
        line = _LIST_MARKER.sub("", line, count=1).strip()
        pos = 0
        for m in _SENTENCE_END.finditer(line):
            out.append(line[pos:m.end()].strip())
            pos = m.end()
        out.append(line[pos:].strip())
    # what holds no word outside its citations (an empty rest, a stray bracket) is not a sentence
    return [s for s in out if re.search(r"\w", _CITE.sub("", s))]


def validate_citations(text: str, evidence_ids: Sequence[str]) -> Dict[str, Any]:
    """{"valid", "sentences", "uncited": [sentence], "unknown_ids": [id], "cited": [id in order of first use]}: a
    sentence passes when it cites at least one id and every id it cites is in the pack."""
    known = {str(e) for e in evidence_ids}
    sentences = split_sentences(text or "")
    uncited: List[str] = []
    unknown: List[str] = []
    cited: List[str] = []
    for s in sentences:
        ids = [_normal_id(a, b) for a, b in _CITE.findall(s)]
        if not ids:
            uncited.append(s)
        for i in ids:
            if i not in known:
                if i not in unknown:
                    unknown.append(i)
            elif i not in cited:
                cited.append(i)
    # ids outside any sentence (a line of brackets alone) are checked as well
    for a, b in _CITE.findall(text or ""):
        i = _normal_id(a, b)
        if i not in known and i not in unknown:
            unknown.append(i)
    return {"valid": bool(sentences) and not uncited and not unknown, "sentences": len(sentences), "uncited": uncited,
            "unknown_ids": unknown, "cited": cited}


# ---- the LLM call -----------------------------------------------------------------------------------------------
def _post_json(url: str, headers: Dict[str, str], body: Dict[str, Any], timeout_s: float) -> Tuple[int, str]:
    """The one place a socket is opened: (status code, response text)."""
    import httpx  # only needed for the http path

    try:
        with httpx.Client(timeout=httpx.Timeout(timeout_s)) as client:
            resp = client.post(url, json=body, headers=headers)
    except httpx.HTTPError as exc:
        raise AnswerClientError(f"LLM HTTP request failed: {exc}") from exc
    return resp.status_code, resp.text


def _chat_http(messages: List[Dict[str, str]], max_new_tokens: int, sampling: Optional[SamplingParams] = None,
               penalties: Optional[PenaltyParams] = None) -> Tuple[str, str]:
    import json

    url = settings.llm_base_url.rstrip("/") + "/chat/completions"
    headers = {"Authorization": f"Bearer {settings.llm_api_key}"} if settings.llm_api_key else {}
    body = {"model": settings.llm_model, "messages": messages, "temperature": 0, "max_tokens": int(max_new_tokens)}
    if sampling is not None:   # the three knobs every OpenAI-compatible service knows
        body.update(temperature=float(sampling.temperature), top_p=float(sampling.top_p), seed=int(sampling.seed))
    if penalties is not None:  # ... and the three of these; the others are no part of the protocol (penalties_ignored)
        body.update(presence_penalty=float(penalties.presence_penalty),
                    frequency_penalty=float(penalties.frequency_penalty))
        if penalties.logit_bias:   # the protocol's range is -100..100: -inf goes as its lower end
            body["logit_bias"] = {str(t): max(float(b), -100.0) for t, b in penalties.logit_bias.items()}
    status, text = _post_json(url, headers, body, settings.llm_timeout_s)
    if status != 200:
        raise AnswerClientError(f"LLM service returned {status}: {text.strip()[:400]}")
    try:
        payload = json.loads(text)
        content = payload["choices"][0]["message"]["content"]
    except (ValueError, KeyError, IndexError, TypeError) as exc:
        raise AnswerClientError(f"LLM response is not a chat completion: {exc}") from exc
    if not isinstance(content, str):
        raise AnswerClientError("LLM response holds no text")
    return content, str(payload.get("model") or settings.llm_model)


def _chat_native(messages: List[Dict[str, str]], max_new_tokens: int, grammar: Optional[TokenGrammar] = None,
                 sampling: Optional[SamplingParams] = None, stream: int = 0, speculate: int = 0,
                 logprobs: Optional[int] = None, penalties: Optional[PenaltyParams] = None) -> Tuple[str, str]:
    """ValueError (the prompt does not fit) passes through to the caller, which drops evidence."""
    llm = _llm
    if llm is None:
        raise AnswerClientError("native LLM is not loaded (call set_llm)")
    try:
        with _llm_lock:
            extra: Dict[str, Any] = {} if grammar is None else {"grammar": grammar}
            if sampling is not None:
                extra.update(sampling=sampling, stream=int(stream))
            if speculate:
                extra.update(speculate=int(speculate))
            if logprobs is not None:
                extra.update(logprobs=int(logprobs))
            extra.update(_penalty_kwargs(llm, penalties))
            text = llm.generate_text(messages, max_new_tokens, **extra)
    except (AnswerClientError, ValueError):
        raise
    except Exception as exc:  # noqa: BLE001 - callers rely on a single error type
        raise AnswerClientError(f"native LLM failed: {exc}") from exc
    if not isinstance(text, str):
        raise AnswerClientError("native LLM returned no text")
    return text, str(getattr(llm, "model_id", None) or settings.llm_model)


def chat_samples(messages: List[Dict[str, str]], n: int, max_new_tokens: Optional[int] = None,
                 grammar: Optional[TokenGrammar] = None, sampling: Optional[SamplingParams] = None,
                 streams: Optional[Sequence[int]] = None, speculate: int = 0, logprobs: Optional[int] = None,
                 penalties: Optional[PenaltyParams] = None) -> Tuple[List[str], str]:
    """(n replies, model id) from the registered native model's generate_text_samples (native_samples()).  ValueError
    (the prompt does not fit) passes through, as from chat().  speculate > 0: a model with supports_speculation only; logprobs: one with supports_logprobs only."""
    llm = _llm
    if not llm_enabled() or not _is_native(settings.llm_base_url) or llm is None:
        raise AnswerClientError("native LLM is not loaded (call set_llm)")
    try:
        with _llm_lock:
            texts = llm.generate_text_samples(messages, int(n), int(max_new_tokens or settings.llm_max_new_tokens),
                                              grammar=grammar, sampling=sampling,
                                              streams=None if streams is None else [int(x) for x in streams],
                                              **({"speculate": int(speculate)} if speculate else {}),
                                              **({} if logprobs is None else {"logprobs": int(logprobs)}),
                                              **_penalty_kwargs(llm, penalties))
    except (AnswerClientError, ValueError):
        raise
    except Exception as exc:  # noqa: BLE001 - callers rely on a single error type
        raise AnswerClientError(f"native LLM failed: {exc}") from exc
    if not isinstance(texts, list) or len(texts) != int(n) or not all(isinstance(t, str) for t in texts):
        raise AnswerClientError(f"native LLM did not return {int(n)} texts")
    return texts, str(getattr(llm, "model_id", None) or settings.llm_model)


def chat(messages: List[Dict[str, str]], max_new_tokens: Optional[int] = None, grammar: Optional[TokenGrammar] = None,
         sampling: Optional[SamplingParams] = None, stream: int = 0, speculate: int = 0,
         logprobs: Optional[int] = None, penalties: Optional[PenaltyParams] = None) -> Tuple[str, str]:
    """(reply, model id) from the configured LLM.  grammar: native backend only (an HTTP service cannot take one).
    speculate > 0: native backend only, a model with supports_speculation (native_speculation()).
    sampling: None is greedy; a native model must have supports_sampling (native_sampling()), and draws on noise stream
    `stream`; an HTTP service gets temperature, top_p and seed.
    logprobs: native backend only, a model with supports_logprobs (native_logprobs()); its records are in the model's
    last_logprobs.
    penalties: a native model must have supports_penalties (native_penalties()) and takes all of it, with the citation
    alphabet exempt; an HTTP service gets presence_penalty, frequency_penalty and logit_bias."""
    if not llm_enabled():
        raise AnswerClientError("LLM_BASE_URL is not configured")
    budget = int(max_new_tokens or settings.llm_max_new_tokens)
    if _is_native(settings.llm_base_url):
        return _chat_native(messages, budget, grammar, sampling, stream, speculate, logprobs, penalties)
    return _chat_http(messages, budget, sampling, penalties)


def constrained_decoding() -> bool:
    """ANSWER_CONSTRAINED applies: it is on, the backend is native and the registered model takes a grammar."""
    return bool(settings.answer_constrained) and _is_native(settings.llm_base_url) \
        and bool(getattr(_llm, "supports_grammar", False))


def native_sampling() -> bool:
    """The registered native model takes sampling=SamplingParams."""
    return bool(getattr(_llm, "supports_sampling", False))


def native_samples() -> bool:
    """The backend is native and the registered model has generate_text_samples."""
    return _is_native(settings.llm_base_url) and bool(getattr(_llm, "supports_samples", False))


def native_speculation() -> bool:
    """The backend is native and the registered model takes speculate=k."""
    return _is_native(settings.llm_base_url) and bool(getattr(_llm, "supports_speculation", False))


def native_logprobs() -> bool:
    """The backend is native and the registered model takes logprobs=n."""
    return _is_native(settings.llm_base_url) and bool(getattr(_llm, "supports_logprobs", False))


def native_penalties() -> bool:
    """The backend is native and the registered model takes penalties=PenaltyParams."""
    return _is_native(settings.llm_base_url) and bool(getattr(_llm, "supports_penalties", False))


_PENALTY_FIELDS = ("repetition_penalty", "presence_penalty", "frequency_penalty", "no_repeat_ngram", "logit_bias",
                   "min_new_tokens")
_HTTP_PENALTY_FIELDS = ("presence_penalty", "frequency_penalty", "logit_bias")


def penalties_for(request: Any) -> Optional[PenaltyParams]:
    """The request's repetition-control fields over the ANSWER_* defaults; None when the result is neutral -- decoding
    is then exactly what it is without them.  AnswerRequestError: a value out of range."""
    import json

    merged = {}
    for name in _PENALTY_FIELDS:
        given = getattr(request, name, None)
        merged[name] = getattr(settings, "answer_" + name) if given is None else given
    try:
        if isinstance(merged["logit_bias"], str):   # the setting: a JSON object as text
            merged["logit_bias"] = json.loads(merged["logit_bias"]) if merged["logit_bias"].strip() else {}
        return _active_penalties(PenaltyParams(**merged))
    except (TypeError, ValueError) as exc:
        raise AnswerRequestError(str(exc)) from exc


def _penalty_kwargs(llm: Any, penalties: Optional[PenaltyParams]) -> Dict[str, Any]:
    """What a native model with supports_penalties is passed: the parameters, and the ids of the citation alphabet as
    exempt -- citing [Q-12] a second time is never penalised or banned -- when the model has a token table."""
    if penalties is None:
        return {}
    table = getattr(llm, "token_table", None)
    return {"penalties": penalties,
            "penalty_exempt": exempt_ids(table(), CITATION_ALPHABET) if callable(table) else None}


def logprobs_for(request: Any) -> bool:
    """The request's `logprobs` over ANSWER_LOGPROBS."""
    given = getattr(request, "logprobs", None)
    return bool(settings.answer_logprobs if given is None else given)


def sample_rank_for(request: Any) -> str:
    """The request's `sample_rank` over ANSWER_SAMPLE_RANK.  AnswerRequestError: neither "first" nor "logprob"."""
    given = getattr(request, "sample_rank", None)
    rank = settings.answer_sample_rank if given is None else given
    if rank not in ("first", "logprob"):
        raise AnswerRequestError(f'sample_rank must be "first" or "logprob" (got {rank!r})')
    return rank


def speculate_for(request: Any) -> int:
    """The request's `speculate` over ANSWER_SPECULATE: drafted tokens verified per forward.  AnswerRequestError: outside
    0..7."""
    given = getattr(request, "speculate", None)
    k = settings.answer_speculate if given is None else given
    if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= 7:
        raise AnswerRequestError(f"speculate must be an integer in 0..7 (got {k!r})")
    return k


def samples_for(request: Any) -> int:
    """The request's `samples` over ANSWER_SAMPLES: how many candidates an attempt draws.  AnswerRequestError: outside
    1..8, or more than one while decoding is greedy (sampling_for gives None) -- n greedy copies are one answer."""
    given = getattr(request, "samples", None)
    n = settings.answer_samples if given is None else given
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= 8:
        raise AnswerRequestError(f"samples must be an integer in 1..8 (got {n!r})")
    sampling = sampling_for(request) if n > 1 else None
    if n > 1 and (sampling is None or float(sampling.temperature) == 0.0):   # (a named temperature of 0 is greedy too)
        raise AnswerRequestError(f"samples = {n} needs sampling: with a temperature of 0 every candidate is the same answer")
    return n


def sampling_for(request: Any) -> Optional[SamplingParams]:
    """The request's sampling fields over the ANSWER_* defaults.  None -- greedy decoding, exactly as without sampling --
    when the temperature comes out 0 and the request names no sampling field.  AnswerRequestError: a value out of range."""
    given = {name: getattr(request, name, None) for name in ("temperature", "top_p", "top_k", "min_p", "seed")}
    base = {"temperature": settings.answer_temperature, "top_p": settings.answer_top_p, "top_k": settings.answer_top_k,
            "min_p": settings.answer_min_p, "seed": settings.answer_seed}
    merged = {name: base[name] if value is None else value for name, value in given.items()}
    if float(merged["temperature"]) == 0.0 and all(value is None for value in given.values()):
        return None
    try:
        return SamplingParams(**merged)
    except (TypeError, ValueError) as exc:
        raise AnswerRequestError(str(exc)) from exc


def _grammar_for(items: Sequence[Dict[str, Any]], notes: Dict[str, Any]) -> Optional[TokenGrammar]:
    """The citation grammar of the items in the prompt; None (and the reason in the notes) when it cannot be built."""
    try:
        dfa = citation_grammar([i["evidence_id"] for i in items])
    except ValueError as exc:
        notes["constrained"] = False
        notes["constrained_error"] = str(exc)
        return None
    table = getattr(_llm, "token_table", None)
    notes["constrained"] = True
    return TokenGrammar(dfa, table() if callable(table) else None)


# ---- /answer ----------------------------------------------------------------------------------------------------
@dataclass
class AnswerRequest(_retrieve.RetrieveRequest):
    """The /retrieve request plus echo_evidence, the optional sampling fields, `samples`, the candidates per attempt, and
    `speculate`, the drafts per forward, `logprobs` and `sample_rank` (None: the ANSWER_* default)."""
    echo_evidence: bool = False
    temperature: Optional[float] = None
    top_p: Optional[float] = None
    top_k: Optional[int] = None
    min_p: Optional[float] = None
    seed: Optional[int] = None
    samples: Optional[int] = None
    speculate: Optional[int] = None
    logprobs: Optional[bool] = None
    sample_rank: Optional[str] = None
    repetition_penalty: Optional[float] = None
    presence_penalty: Optional[float] = None
    frequency_penalty: Optional[float] = None
    no_repeat_ngram: Optional[int] = None
    logit_bias: Optional[Dict[Any, float]] = None
    min_new_tokens: Optional[int] = None


def _evidence_items(pack: Dict[str, Any]) -> List[Dict[str, Any]]:
    """The pack's items in rank order: artifacts, then quotes (the order _pack fills them in)."""
    return list(pack.get("artifacts") or []) + list(pack.get("quotes") or [])


def _item_line(item: Dict[str, Any]) -> str:
    who = item.get("speaker") or item.get("kind") or "source"
    return f"[{item['evidence_id']}] {who}: {item.get('snippet', '')}"


def build_messages(query: str, items: Sequence[Dict[str, Any]], turns: Sequence[Dict[str, str]] = ()
                   ) -> List[Dict[str, str]]:
    evidence = "\n".join(_item_line(i) for i in items)
    user = f"Evidence:\n{evidence}\n\nQuestion: {query}\n\nAnswer from the evidence only, citing every sentence."
    return [{"role": "system", "content": SYSTEM_RULES}, {"role": "user", "content": user}, *turns]


def _repair_message(report: Dict[str, Any], ids: Sequence[str]) -> str:
    parts = ["Your answer failed the citation check."]
    if report["uncited"]:
        parts.append("These sentences cite no evidence id: " + " | ".join(report["uncited"]))
    if report["unknown_ids"]:
        parts.append("These ids are not in the evidence: " + ", ".join(report["unknown_ids"]))
    if not report["sentences"]:
        parts.append("The answer held no sentence.")
    parts.append("Allowed ids: " + ", ".join(f"[{i}]" for i in ids) + ". Rewrite the whole answer so that every sentence "
                 "ends with at least one allowed id, or reply with exactly " + INSUFFICIENT + ".")
    return " ".join(parts)


def answer_question(request: AnswerRequest, backend: Optional[_retrieve.RetrieveBackend] = None) -> Dict[str, Any]:
    if not llm_enabled():
        raise AnswerClientError("LLM_BASE_URL is not configured")
    sampling = sampling_for(request)
    n_samples = samples_for(request)
    speculate = speculate_for(request)
    want_logprobs = logprobs_for(request)
    rank_mode = sample_rank_for(request)
    penalties = penalties_for(request)
    pack_request = _retrieve.RetrieveRequest(query=request.query, intent=request.intent, filters=request.filters,
                                             budget=request.budget, return_style="evidence_pack_json", debug=request.debug,
                                             facets=request.facets, facet_top=request.facet_top)
    pack = _retrieve.retrieve_evidence(pack_request, backend)
    items = _evidence_items(pack)
    notes: Dict[str, Any] = {"evidence_items": len(items), "dropped_evidence": 0, "llm_calls": 0, "validator": None}
    if settings.answer_constrained:     # with the setting off the response is what it always was: no such note
        notes["constrained"] = False    # True once a call has decoded under a grammar
    if sampling is not None:            # greedy by default: no such note
        notes["sampling"] = sampling.echo()
        if _is_native(settings.llm_base_url) and not native_sampling():
            notes["sampling"]["applied"] = False   # the registered model cannot sample: it decodes greedily
            sampling = None
    if penalties is not None:           # neutral by default: no such note
        notes["penalties"] = penalties.echo()
        if _is_native(settings.llm_base_url):
            if not native_penalties():      # the registered model takes none: it decodes as without them
                notes["penalties"]["applied"] = False
                penalties = None
        else:   # an HTTP service is sent the three knobs of its protocol; the others that are set are named here
            ignored = [name for name in _PENALTY_FIELDS if name not in _HTTP_PENALTY_FIELDS
                       and getattr(penalties, name) != getattr(PenaltyParams(), name)]
            if ignored:
                notes["penalties_ignored"] = ignored
    # several candidates come from one call of a native model that can fork a prefill; anything else draws one as ever
    multi = n_samples > 1 and sampling is not None and native_samples()
    if n_samples > 1 and not multi:
        notes["samples"] = {"applied": False}
    if speculate and not native_speculation():   # off by default: no such note
        notes["speculation"] = {"applied": False}
        speculate = 0
    ranked = rank_mode == "logprob" and multi and native_logprobs()
    if rank_mode == "logprob" and not ranked:    # "first" by default: no such entry
        notes["samples"] = dict(notes.get("samples") or {}, ranked=False)
    if want_logprobs and not native_logprobs():  # off by default: no such note
        notes["logprobs"] = {"applied": False}
        want_logprobs = False
    scoring = 0 if (want_logprobs or ranked) else None   # the model's logprobs=: the records, no top entries
    out: Dict[str, Any] = {"query_id": pack["query_id"], "answer": None, "status": STATUS_INSUFFICIENT, "citations": [],
                           "repairs": 0, "model": None, "notes": notes}
    if getattr(request, "echo_evidence", False):
        out["evidence_pack"] = pack
    if not items:
        return out

    turns: List[Dict[str, str]] = []
    query = request.query.strip()

    constrained = constrained_decoding()

    def call(attempt: int) -> Tuple[List[str], Optional[List[list]]]:
        """The candidates of one attempt: one reply, or under `multi` n_samples from one call; and under `scoring` the
        TokenLogprob records of each."""
        while True:
            try:
                # the grammar of the items in THIS prompt: rebuilt when an item has been dropped for length
                grammar = _grammar_for(items, notes) if constrained else None
                if multi:
                    texts, model = chat_samples(build_messages(query, items, turns), n_samples, grammar=grammar,
                                                sampling=sampling,
                                                streams=[attempt * n_samples + i for i in range(n_samples)],
                                                speculate=speculate, logprobs=scoring, penalties=penalties)
                else:
                    extra = {} if sampling is None else {"sampling": sampling, "stream": attempt}
                    if speculate:
                        extra["speculate"] = speculate
                    if scoring is not None:
                        extra["logprobs"] = scoring
                    if penalties is not None:
                        extra["penalties"] = penalties
                    text, model = chat(build_messages(query, items, turns), grammar=grammar, **extra)
                    texts = [text]
            except ValueError as exc:   # the prompt does not fit the model's context: the lowest-ranked item goes
                if len(items) <= 1:
                    raise AnswerClientError(f"the prompt does not fit with a single evidence item: {exc}") from exc
                items.pop()
                notes["dropped_evidence"] += 1
                continue
            notes["llm_calls"] += 1
            out["model"] = model
            # a native generator with a prefix cache says how many prompt tokens it took from its KV cache
            reuse = getattr(_llm, "last_reuse", None) if _is_native(settings.llm_base_url) else None
            if reuse is not None:
                # (under `multi` every candidate reports the one prompt's rows: they were reused once)
                notes["prefix_reused_tokens"] = notes.get("prefix_reused_tokens", 0) + \
                    int(reuse["reused"][0] if multi else sum(reuse["reused"]))
            if speculate:   # what the last call drafted and kept
                notes["speculation"] = getattr(_llm, "last_speculation", None)
            records = None
            if scoring is not None:
                records = getattr(_llm, "last_logprobs", None)
                if not isinstance(records, list) or len(records) != len(texts):
                    raise AnswerClientError(f"native LLM left no token log-probabilities for its {len(texts)} replies")
            return texts, records

    max_repairs = max(int(settings.answer_max_repairs), 0)
    for attempt in range(max_repairs + 1):
        texts, records = call(attempt)
        texts = [t.strip() for t in texts]
        out["repairs"] = attempt
        ids = [i["evidence_id"] for i in items]
        # judged in index order; None: the candidate says INSUFFICIENT_EVIDENCE
        reports = [None if t.strip(" .\"'`*") == INSUFFICIENT else validate_citations(t, ids) for t in texts]
        order = list(range(len(texts)))
        if ranked:   # by mean token log-probability, the lowest index among equals (a reply without a token last)
            scores = [mean_logprob(rec) for rec in records]
            order.sort(key=lambda i: -(scores[i] if scores[i] is not None and scores[i] == scores[i] else float("-inf")))
        chosen = next((i for i in order if reports[i] is not None and reports[i]["valid"]), None)
        if multi:
            notes["samples"] = {"drawn": len(texts), "valid": sum(1 for r in reports if r is not None and r["valid"]),
                                "chosen": chosen}
            if ranked:
                notes["samples"].update(scores=scores, ranked=True)
            elif rank_mode == "logprob":
                notes["samples"]["ranked"] = False
        if want_logprobs:   # of the judged candidate: the chosen one, or the one the repair turn will quote
            judged = chosen if chosen is not None else next((i for i in order if reports[i] is not None), order[0])
            notes["logprobs"] = summarise(records[judged])
        if all(r is None for r in reports):
            out["status"] = STATUS_INSUFFICIENT
            return out
        if chosen is None:   # the repair turn quotes the first candidate, in that order, that tried to answer
            chosen = next(i for i in order if reports[i] is not None)
        text, report = texts[chosen], reports[chosen]
        notes["validator"] = report
        if report["valid"]:
            by_id = {i["evidence_id"]: i for i in items}
            out.update(answer=text, status=STATUS_OK,
                       citations=[{"evidence_id": c, "call_id": by_id[c]["call_id"]} for c in report["cited"]])
            return out
        turns += [{"role": "assistant", "content": text}, {"role": "user", "content": _repair_message(report, ids)}]
    out["status"] = STATUS_FAILED
    return out
