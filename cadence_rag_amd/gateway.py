"""HTTP shim with the reference gateway's contract, so an UNMODIFIED reference app can point
EMBEDDINGS_BASE_URL at the MI355X box: `POST /embed {texts, model?} -> {embeddings, model}` and
`GET /health` (/root/reference/P620_TRITON_QWEN3_4B_EMBEDDING_RUNBOOK.md:489-497,669-716).
The body is served by the in-process encoder registered with embeddings.set_encoder().
`POST /rerank {query, documents, model?} -> {scores, order, model}` is the reranker's contract
(the reference's NVIDIA_IMMERSION_PLAN.md:93-97), served by the reranker registered with reranker.set_reranker().
`POST /answer` (the /retrieve request plus echo_evidence) is the citation-gated answer of answer.answer_question, served
by the LLM registered with answer.set_llm() or the service LLM_BASE_URL names.
`POST /retrieve` is the reference's own route (/root/reference/app/main.py:184-186) over
retrieve.retrieve_evidence and the backend registered with retrieve.set_backend().

    uvicorn cadence_rag_amd.gateway:app --host 0.0.0.0 --port 8100
"""
from __future__ import annotations

from datetime import datetime
from typing import Dict, List, Literal, Optional
from uuid import UUID

from fastapi import FastAPI, HTTPException
from pydantic import BaseModel, Field

from . import answer as _answer
from . import embeddings
from . import reranker
from . import retrieve as _retrieve
from .config import settings


class EmbedRequest(BaseModel):
    texts: List[str] = Field(default_factory=list)
    model: Optional[str] = None


class EmbedResponse(BaseModel):
    embeddings: List[List[float]]
    model: str


app = FastAPI(title="Cadence RAG MI355X embedding gateway")


@app.get("/health")
def health() -> dict:
    enc = embeddings.get_encoder()
    return {"status": "ok" if enc is not None else "degraded", "backend": "mi355x-native",
            "encoder_loaded": enc is not None, "embed_output_dim": settings.embeddings_dim,
            "model": settings.embeddings_model_id, "llm_loaded": _answer.get_llm() is not None}


@app.post("/embed", response_model=EmbedResponse)
def embed(req: EmbedRequest) -> EmbedResponse:
    texts = [t for t in req.texts if isinstance(t, str) and t.strip()]
    if not texts:
        raise HTTPException(status_code=400, detail="texts must contain at least one non-empty string")
    enc = embeddings.get_encoder()
    if enc is None:
        raise HTTPException(status_code=502, detail="native encoder is not loaded")
    try:
        with embeddings._encoder_lock:
            vectors, model = enc.encode(texts)
    except Exception as exc:  # noqa: BLE001
        raise HTTPException(status_code=502, detail=f"encoder failed: {exc}") from exc
    vectors = [[float(x) for x in v] for v in vectors]
    if any(len(v) != settings.embeddings_dim for v in vectors):
        raise HTTPException(status_code=502, detail=f"encoder returned vectors of the wrong size "
                                                    f"(expected {settings.embeddings_dim})")
    return EmbedResponse(embeddings=vectors, model=req.model or model)


class RerankRequest(BaseModel):
    query: str = ""
    documents: List[str] = Field(default_factory=list)
    model: Optional[str] = None


class RerankResponse(BaseModel):
    scores: List[float]
    order: List[int]
    model: str


@app.post("/rerank", response_model=RerankResponse)
def rerank(req: RerankRequest) -> RerankResponse:
    if not req.query.strip():
        raise HTTPException(status_code=400, detail="query must be a non-empty string")
    if not req.documents:
        raise HTTPException(status_code=400, detail="documents must contain at least one string")
    rr = reranker.get_reranker()
    if rr is None:
        raise HTTPException(status_code=502, detail="native reranker is not loaded")
    try:
        with reranker._reranker_lock:
            scores, order, model = rr.rerank(req.query.strip(), list(req.documents))
        res = reranker._validate_result(scores, order, model, len(req.documents))
    except Exception as exc:  # noqa: BLE001
        raise HTTPException(status_code=502, detail=f"reranker failed: {exc}") from exc
    return RerankResponse(scores=res.scores, order=res.order, model=req.model or res.model)


# ---- POST /retrieve: request models field-for-field app/schemas.py:71-93 -------------------------
class BudgetModel(BaseModel):
    max_evidence_items: int = 8
    max_total_chars: int = 6000


class RetrieveFiltersModel(BaseModel):
    date_from: Optional[datetime] = None
    date_to: Optional[datetime] = None
    call_ids: Optional[List[UUID]] = None
    external_id: Optional[str] = None
    external_source: Optional[str] = None
    call_tags: Optional[List[str]] = None
    # row-level filters: [{"label": ..., "value": ...}] ANDed; any of `speakers`; any of `kinds`
    entity_filters: Optional[List[Dict[str, str]]] = None
    speakers: Optional[List[str]] = None
    kinds: Optional[List[str]] = None


class RetrieveRequestModel(BaseModel):
    query: str
    intent: Literal["auto", "decision", "action_items", "who_said", "troubleshooting", "status"] = "auto"
    filters: Optional[RetrieveFiltersModel] = None
    budget: BudgetModel = Field(default_factory=BudgetModel)
    return_style: Literal["evidence_pack_json", "ids_only"] = "evidence_pack_json"
    debug: bool = False
    # facet counts: namespaces to count over the rows that pass `filters`; a violation is a 422
    facets: Optional[List[str]] = Field(default=None, max_length=16)
    facet_top: int = Field(default=10, ge=1, le=64)


def _request_fields(payload: RetrieveRequestModel) -> dict:
    filters = None
    if payload.filters is not None:
        filters = _retrieve.RetrieveFilters(**payload.filters.model_dump())
    return dict(query=payload.query, intent=payload.intent, filters=filters,
                budget=_retrieve.Budget(**payload.budget.model_dump()), return_style=payload.return_style,
                debug=payload.debug, facets=payload.facets, facet_top=payload.facet_top)


@app.post("/retrieve")
def retrieve_endpoint(payload: RetrieveRequestModel) -> dict:
    request = _retrieve.RetrieveRequest(**_request_fields(payload))
    try:
        return _retrieve.retrieve_evidence(request)
    except RuntimeError as exc:  # no backend registered
        raise HTTPException(status_code=503, detail=str(exc)) from exc


class AnswerRequestModel(RetrieveRequestModel):
    echo_evidence: bool = False
    # sampling (cadence_rag_amd.sampling): absent fields take the ANSWER_* defaults; a value out of range is a 422
    temperature: Optional[float] = Field(default=None, ge=0.0, le=100.0)
    top_p: Optional[float] = Field(default=None, gt=0.0, le=1.0)
    top_k: Optional[int] = Field(default=None, ge=0)
    min_p: Optional[float] = Field(default=None, ge=0.0, le=1.0)
    seed: Optional[int] = Field(default=None, ge=0, lt=2 ** 64)
    samples: Optional[int] = Field(default=None, ge=1, le=8)   # candidates per attempt (ANSWER_SAMPLES when absent)
    speculate: Optional[int] = Field(default=None, ge=0, le=7)   # drafts per forward (ANSWER_SPECULATE when absent)
    logprobs: Optional[bool] = None      # score the answer's tokens (ANSWER_LOGPROBS when absent)
    sample_rank: Optional[str] = None    # "first" or "logprob" (ANSWER_SAMPLE_RANK when absent); anything else is a 422
    # repetition control (cadence_rag_amd.penalties): absent fields take the ANSWER_* defaults; out of range is a 422
    repetition_penalty: Optional[float] = Field(default=None, ge=0.1, le=10.0)
    presence_penalty: Optional[float] = Field(default=None, ge=-2.0, le=2.0)
    frequency_penalty: Optional[float] = Field(default=None, ge=-2.0, le=2.0)
    no_repeat_ngram: Optional[int] = Field(default=None, ge=0, le=8)
    logit_bias: Optional[Dict[str, float]] = None    # token id -> value in -100..100, or -inf (checked by PenaltyParams)
    min_new_tokens: Optional[int] = Field(default=None, ge=0)


@app.post("/answer")
def answer_endpoint(payload: AnswerRequestModel) -> dict:
    request = _answer.AnswerRequest(**_request_fields(payload), echo_evidence=payload.echo_evidence,
                                    temperature=payload.temperature, top_p=payload.top_p, top_k=payload.top_k,
                                    min_p=payload.min_p, seed=payload.seed, samples=payload.samples,
                                    speculate=payload.speculate, logprobs=payload.logprobs,
                                    sample_rank=payload.sample_rank, repetition_penalty=payload.repetition_penalty,
                                    presence_penalty=payload.presence_penalty,
                                    frequency_penalty=payload.frequency_penalty, no_repeat_ngram=payload.no_repeat_ngram,
                                    logit_bias=payload.logit_bias, min_new_tokens=payload.min_new_tokens)
    try:
        return _answer.answer_question(request)
    except _answer.AnswerRequestError as exc:
        raise HTTPException(status_code=422, detail=str(exc)) from exc
    except _answer.AnswerClientError as exc:
        raise HTTPException(status_code=502, detail=str(exc)) from exc
    except RuntimeError as exc:  # no retrieve backend registered
        raise HTTPException(status_code=503, detail=str(exc)) from exc
