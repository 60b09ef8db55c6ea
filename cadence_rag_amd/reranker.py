"""Rerank client seam, the counterpart of embeddings.py for the reference's Phase-4 stage ("RRF -> GPU rerank top N
-> top M", PHASED_PLAN.md:286-310): RerankClientError, RerankResult, rerank_enabled, rerank_texts.

RERANK_BASE_URL="" turns reranking off; "native" (or "native://...") routes to the in-process reranker registered
with set_reranker() (cadence_rag_amd.encoder.rerank.Qwen3Reranker); an http(s) URL speaks the gateway contract
`POST /rerank {query, documents, model} -> {scores, order, model}` (NVIDIA_IMMERSION_PLAN.md:93-97).  Every failure
reaches the caller as RerankClientError, and every answer is validated before it is returned (fail closed).
"""
from __future__ import annotations

import math
import threading
from dataclasses import dataclass
from typing import List, Optional, Protocol, Sequence, Tuple

from .config import settings


class RerankClientError(RuntimeError):
    pass


@dataclass(frozen=True)
class RerankResult:
    scores: List[float]   # one per document, input order
    order: List[int]      # document indices by descending score (ties: input order)
    model: str


class Reranker(Protocol):
    """In-process backend: (query, documents) -> (scores, order, model id).  May raise any exception; it is
    reported as RerankClientError."""

    def rerank(self, query: str, documents: Sequence[str]) -> Tuple[Sequence[float], Sequence[int], str]: ...


_reranker: Optional[Reranker] = None
_reranker_lock = threading.Lock()  # one GPU submission at a time (FastAPI runs sync endpoints on a threadpool)


def set_reranker(reranker: Optional[Reranker]) -> None:
    global _reranker
    _reranker = reranker


def get_reranker() -> Optional[Reranker]:
    return _reranker


def rerank_enabled() -> bool:
    return bool(settings.rerank_base_url.strip())


def _is_native(url: str) -> bool:
    return url.strip().lower().startswith("native")


def _validate_input(query: str, documents: Sequence[str]) -> Tuple[str, List[str]]:
    if not isinstance(query, str) or not query.strip():
        raise RerankClientError("rerank request requires a non-empty query")
    if isinstance(documents, str) or not documents:
        raise RerankClientError("rerank request requires at least one document")
    if any(not isinstance(d, str) for d in documents):
        raise RerankClientError("rerank documents must be strings")
    cut = settings.rerank_max_chars_per_doc
    return query.strip(), [d[:cut] if cut > 0 else d for d in documents]


def _validate_result(scores, order, model, n: int) -> RerankResult:
    try:
        vals = [float(s) for s in scores]
    except (TypeError, ValueError) as exc:
        raise RerankClientError(f"rerank scores are not numbers: {exc}") from exc
    if len(vals) != n:
        raise RerankClientError(f"rerank response count mismatch: got {len(vals)}, expected {n}")
    if not all(math.isfinite(v) for v in vals):
        raise RerankClientError("rerank response holds a non-finite score")
    want = sorted(range(n), key=lambda i: (-vals[i], i))
    if order is None:
        order = want
    try:
        order = [int(i) for i in order]
    except (TypeError, ValueError) as exc:
        raise RerankClientError(f"rerank order is not a list of indices: {exc}") from exc
    if sorted(order) != list(range(n)):
        raise RerankClientError("rerank order is not a permutation of the documents")
    if any(vals[a] < vals[b] for a, b in zip(order, order[1:])):
        raise RerankClientError("rerank order does not follow the scores")
    return RerankResult(scores=vals, order=order, model=str(model or settings.rerank_model_id))


def _rerank_native(query: str, documents: List[str]):
    rr = _reranker
    if rr is None:
        raise RerankClientError("native reranker is not loaded (call set_reranker)")
    try:
        with _reranker_lock:
            return rr.rerank(query, documents)
    except RerankClientError:
        raise
    except Exception as exc:  # noqa: BLE001 - callers rely on a single error type
        raise RerankClientError(f"native reranker failed: {exc}") from exc


def _rerank_http(query: str, documents: List[str]):
    import httpx  # only needed for the gateway path

    url = settings.rerank_base_url.rstrip("/") + "/rerank"
    body = {"query": query, "documents": documents, "model": settings.rerank_model_id}
    try:
        with httpx.Client(timeout=httpx.Timeout(settings.rerank_timeout_s)) as client:
            resp = client.post(url, json=body)
    except httpx.HTTPError as exc:
        raise RerankClientError(f"rerank HTTP request failed: {exc}") from exc
    if resp.status_code != 200:
        detail = resp.text.strip()[:400]
        raise RerankClientError(f"rerank service returned {resp.status_code}: {detail}")
    try:
        payload = resp.json()
    except ValueError as exc:
        raise RerankClientError(f"rerank response is not JSON: {exc}") from exc
    if not isinstance(payload, dict) or not isinstance(payload.get("scores"), list):
        raise RerankClientError("rerank response missing 'scores' list")
    return payload["scores"], payload.get("order"), payload.get("model")


def rerank_texts(query: str, documents: Sequence[str]) -> RerankResult:
    if not rerank_enabled():
        raise RerankClientError("RERANK_BASE_URL is not configured")
    query, docs = _validate_input(query, documents)
    if _is_native(settings.rerank_base_url):
        scores, order, model = _rerank_native(query, docs)
    else:
        scores, order, model = _rerank_http(query, docs)
    return _validate_result(scores, order, model, len(docs))
