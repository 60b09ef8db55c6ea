"""Dense lane of /retrieve — the counterpart of the dense helpers in the reference's
app/retrieve.py (/root/reference/app/retrieve.py:245-389): _vector_literal, _dense_has_scoping,
_choose_dense_mode, _estimate_dense_candidates, _fetch_chunks_dense, _fetch_artifacts_dense and
_rrf_merge, with the same argument meaning and row shapes.  The SQL + pgvector scan is replaced by
a DenseTable: a DenseIndex in HBM plus the per-row columns the reference SELECTs, kept on the host.
Filters (_build_filter_clause, retrieve.py:93-120) become a row bitmask handed to the scan kernel.

The orchestrator (retrieve_evidence), the BM25 and tech-token lanes and the evidence-pack shaping
stay in the reference app; INTEGRATION.md shows the three call sites that switch to this module.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from datetime import datetime
from typing import Any, Dict, List, Optional, Sequence, Set, Tuple, Union
from uuid import UUID

import numpy as np

from .config import settings
from .dense_index import DenseIndex
from .snippets import clip as _clip, cut_snippet   # (_clip: the head clip of retrieve.py:24-29)

_log = logging.getLogger(__name__)

DEFAULT_RRF_K = 60
DEFAULT_DENSE_CHUNK_TOPK = 50
DEFAULT_DENSE_ARTIFACT_CHUNK_TOPK = 10


@dataclass
class RetrieveFilters:
    """Field-for-field the reference's pydantic RetrieveFilters (app/schemas.py:76-82)."""
    date_from: Optional[datetime] = None
    date_to: Optional[datetime] = None
    call_ids: Optional[List[UUID]] = None
    external_id: Optional[str] = None
    external_source: Optional[str] = None
    call_tags: Optional[List[str]] = None
    # row-level filters, planned by the reference (PHASED_PLAN.md:355-380, APP_SPEC.md:616-619) and its own here
    # (DESIGN.md 4.13): every {"label", "value"} entry must be among the row's entities; the row's speaker is one of
    # `speakers`; its kind is one of `kinds`
    entity_filters: Optional[List[Dict[str, str]]] = None
    speakers: Optional[List[str]] = None
    kinds: Optional[List[str]] = None


def _resolve_call_ids(calls: Sequence[Dict[str, Any]], filters: Optional[RetrieveFilters]
                      ) -> Optional[List[UUID]]:
    """external_id (+ external_source) -> call ids, intersected with filters.call_ids
    (/root/reference/app/retrieve.py:46-90).  `calls` stands in for the `calls` table: dicts with
    call_id, external_id, external_source.  None means "no call scoping"; [] means "matches nothing"."""
    if not filters:
        return None
    call_ids: Optional[Set[UUID]] = set(filters.call_ids) if filters.call_ids else None
    if filters.external_id:
        resolved = {c["call_id"] for c in calls
                    if c.get("external_id") == filters.external_id
                    and (filters.external_source is None or c.get("external_source") == filters.external_source)}
        call_ids = (call_ids & resolved) if call_ids else resolved
    if call_ids is None:
        return None
    return sorted(call_ids, key=str)


def _rrf_merge(lanes: Dict[str, Sequence[Dict[str, Any]]], key_field: str, k: int = DEFAULT_RRF_K
               ) -> List[Tuple[Dict[str, Any], Set[str], float]]:
    """Reciprocal-rank fusion: score += 1/(k + rank), rank from 1; the first row seen for a key is
    kept; stable descending sort, so ties keep first-insertion order (lane order of the dict)."""
    score: Dict[Any, float] = {}
    first_row: Dict[Any, Dict[str, Any]] = {}
    hits: Dict[Any, Set[str]] = {}
    for lane, rows in lanes.items():
        for rank, row in enumerate(rows, start=1):
            key = row[key_field]
            score[key] = score.get(key, 0.0) + 1.0 / (k + rank)
            first_row.setdefault(key, row)
            hits.setdefault(key, set()).add(lane)
    order = sorted(score.items(), key=lambda kv: kv[1], reverse=True)
    return [(first_row[key], hits[key], s) for key, s in order]


def _vector_literal(values: Sequence[float]) -> str:
    return "[" + ",".join(format(float(v), ".10g") for v in values) + "]"


def _parse_vector(query_embedding: Union[str, Sequence[float], np.ndarray]) -> np.ndarray:
    if isinstance(query_embedding, str):
        body = query_embedding.strip()
        if not (body.startswith("[") and body.endswith("]")):
            raise ValueError("vector literal must look like '[v0,v1,...]'")
        return np.array([float(x) for x in body[1:-1].split(",")], dtype=np.float32)
    return np.asarray(query_embedding, dtype=np.float32)


def _dense_has_scoping(filters: Optional[RetrieveFilters], call_ids: Optional[Sequence[UUID]]) -> bool:
    if call_ids is not None:
        return True
    if not filters:
        return False
    return bool(filters.date_from or filters.date_to or filters.call_tags or _has_attr_filters(filters))


def _has_attr_filters(filters: Optional[RetrieveFilters]) -> bool:
    """The request carries a row-level clause (entity_filters, speakers or kinds; a falsy field is not applied)."""
    return bool(filters) and bool(getattr(filters, "entity_filters", None) or getattr(filters, "speakers", None)
                                  or getattr(filters, "kinds", None))


def _choose_dense_mode(estimated_rows: int, filters: Optional[RetrieveFilters],
                       call_ids: Optional[Sequence[UUID]]) -> str:
    """The reference's planner string.  The GPU lane always scans exactly; the function is kept so
    `notes.retrieval.dense_modes` keeps its meaning ("exact" / "ann" = what pgvector would do)."""
    if estimated_rows <= 0:
        return "exact"
    if _dense_has_scoping(filters, call_ids) and estimated_rows <= max(settings.embeddings_exact_scan_threshold, 0):
        return "exact"
    return "ann"


class DenseTable:
    """One embedded table (chunks or artifact_chunks): vectors in HBM + the SELECTed columns.

    columns: dict name -> sequence (one entry per row, same order as the vectors), must contain
    `id_field` and "call_id".  call_started_at: per-row datetime/np.datetime64 (the denormalised
    chunks.call_started_at column); call_tags: {call_id: [tags]} (calls.tags, joined on demand).
    """

    def __init__(self, name: str, id_field: str, *, dim: Optional[int] = None, capacity: int = 1 << 16,
                 device: Optional[int] = None) -> None:
        self.name = name
        self.id_field = id_field
        self.index = DenseIndex(dim or settings.embeddings_dim, capacity=capacity,
                                device=settings.embeddings_device if device is None else device)
        self.columns: Dict[str, list] = {}
        self.call_started_at = np.empty((0,), dtype="datetime64[us]")
        self.call_ids = np.empty((0,), dtype=object)
        self.call_tags: Dict[Any, Sequence[str]] = {}
        # bumped whenever rows are appended, removed or move: whatever is built over row POSITIONS (the exact-token lane,
        # packed masks) is stale once it differs
        self.generation = 0
        # per-row tech_tokens (the `tech_tokens text[]` column), kept once a tech lane was built so that the lane
        # can be rebuilt when the table changes; None = not tracked
        self.tech_tokens: Optional[List[List[str]]] = None
        # per-row entities ((label, value) pairs), tracked from the first batch that carries `columns["entities"]`;
        # None = never tracked: the entity namespaces are NULL in this table
        self.entities: Optional[List[List[Tuple[Any, Any]]]] = None
        self._attr_cols = None
        self._facet_cols = None   # filters.FacetColumns, built by the first facet request of a generation
        # device filter columns (cadence_rag_amd.filters), built on first use per generation, and the one mask the
        # lanes of a request share
        self._filter_cols = None
        self._mask_memo: Optional[Tuple[Any, Any]] = None

    def __len__(self) -> int:
        return len(self.index)

    def close(self) -> None:
        for cols in (self._filter_cols, self._attr_cols):
            if cols is not None:
                cols.close()
        self._filter_cols = self._attr_cols = self._facet_cols = self._mask_memo = None
        self.index.close()

    def _take_tokens(self, columns: Dict[str, Sequence[Any]], n: int) -> Tuple[Dict[str, Sequence[Any]], List[List[str]]]:
        """Split an optional "tech_tokens" entry off the SELECTed columns (it feeds the exact-token lane, it is not
        a response column)."""
        if "tech_tokens" not in columns:
            return columns, [[] for _ in range(n)]
        columns = dict(columns)
        toks = [list(t or []) for t in columns.pop("tech_tokens")]
        if len(toks) != n:
            raise ValueError("tech_tokens must have one entry per vector")
        return columns, toks

    def _take_entities(self, columns: Dict[str, Sequence[Any]], n: int
                       ) -> Tuple[Dict[str, Sequence[Any]], Optional[List[List[Tuple[Any, Any]]]]]:
        """Split an optional "entities" entry off the SELECTed columns the way `_take_tokens` splits "tech_tokens": per
        row a list of (label, value) pairs or {"label", "value"} dicts (the chunk_entities / artifact_entities join).
        None when the batch carries none."""
        if "entities" not in columns:
            return columns, None
        from .filters import _entity_pair
        columns = dict(columns)
        ents = [[tuple(_entity_pair(e)) for e in (listed or ())] for listed in columns.pop("entities")]
        if len(ents) != n:
            raise ValueError("entities must have one entry per vector")
        return columns, ents

    def _new_entities(self, n_old: int, ents: Optional[List[List[Tuple[Any, Any]]]], n: int
                      ) -> Optional[List[List[Tuple[Any, Any]]]]:
        """The entities n new rows contribute, or None while the table tracks none: tracking starts with the first batch
        that carries them (the n_old stored rows then hold []), a later batch without them contributes [] per row."""
        if ents is not None and self.entities is None:
            self.entities = [[] for _ in range(n_old)]
        if self.entities is None:
            return None
        return ents if ents is not None else [[] for _ in range(n)]

    def add(self, vectors, columns: Dict[str, Sequence[Any]], call_started_at: Optional[Sequence[Any]] = None,
            call_tags: Optional[Dict[Any, Sequence[str]]] = None) -> None:
        """Append rows whose ids are ascending and above every stored id (the C ABI's contract); the
        index grows when its capacity is exhausted.  Rows that may arrive out of id order go through
        `insert`.  `columns` may carry "tech_tokens" (per-row token lists) for the exact-token lane and "entities"
        (per-row lists of (label, value) pairs or {"label", "value"} dicts) for the entity filters."""
        n = len(columns[self.id_field])
        columns, toks = self._take_tokens(columns, n)
        columns, ents = self._take_entities(columns, n)
        n_old = len(self.call_ids)
        if any(len(v) != n for v in columns.values()):
            raise ValueError("all columns must have one entry per vector")
        ids = np.asarray(columns[self.id_field], dtype=np.int64)
        self._reserve(n)
        self.index.add(vectors, ids=ids)
        for key, vals in columns.items():
            self.columns.setdefault(key, []).extend(list(vals))
        self.call_ids = np.concatenate([self.call_ids, np.asarray(list(columns["call_id"]), dtype=object)])
        ts = (np.asarray(list(call_started_at), dtype="datetime64[us]") if call_started_at is not None
              else np.full((n,), np.datetime64("NaT"), dtype="datetime64[us]"))
        self.call_started_at = np.concatenate([self.call_started_at, ts])
        if call_tags:
            self.call_tags.update(call_tags)
        if self.tech_tokens is not None:
            self.tech_tokens.extend(toks)
        ents = self._new_entities(n_old, ents, n)
        if ents is not None:
            self.entities.extend(ents)
        self._pos_of_id = None
        self.generation += 1

    def _reserve(self, n_more: int) -> None:
        """Make room for n_more rows: the HBM index has a fixed capacity, so a full one is replaced by a
        larger one (x1.5) and the rows move device-to-device."""
        need = len(self.index) + int(n_more)
        if need <= self.index.capacity:
            return
        self._rebuild(capacity=max(need, int(self.index.capacity * 1.5) + 1024))

    def _rebuild(self, capacity: int) -> None:
        """New index of `capacity` rows holding the current rows (device to device)."""
        import torch
        old, n_old = self.index, len(self.index)
        dev = torch.device("cuda", old.device)
        new = DenseIndex(old.dim, capacity=capacity, device=old.device)
        try:
            step = 65536
            for lo in range(0, n_old, step):
                m = min(step, n_old - lo)
                buf = torch.empty(m, old.dim, dtype=torch.float32, device=dev)
                ids = old.get_rows_into(lo, m, buf)
                new.add(buf, ids=ids)
        except Exception:
            new.close()
            raise
        self.index = new
        old.close()
        self.generation += 1

    def insert(self, vectors, columns: Dict[str, Sequence[Any]], call_started_at: Optional[Sequence[Any]] = None,
               call_tags: Optional[Dict[Any, Sequence[str]]] = None) -> None:
        """`add` for rows in any id order (a row embedded late has an id below the stored maximum): when the
        new ids do not simply continue the stored ones, the index moves the rows behind them up in place
        (DenseIndex.insert) and the host columns are merged in ascending id order, which is the order every
        tie-break of the lane assumes.  The index object changes only when its capacity has to grow (`_reserve`).
        An id that is already stored is an error (use DenseIndex.update to re-embed in place)."""
        new_ids = np.asarray(columns[self.id_field], dtype=np.int64)
        n = int(new_ids.size)
        if n == 0:
            return
        old_ids = np.asarray(self.columns.get(self.id_field, []), dtype=np.int64)
        if (old_ids.size == 0 or new_ids.min() > old_ids[-1]) and np.all(np.diff(new_ids) > 0):
            return self.add(vectors, columns, call_started_at, call_tags)
        columns, toks = self._take_tokens(columns, n)
        columns, ents = self._take_entities(columns, n)
        if any(len(v) != n for v in columns.values()):
            raise ValueError("all columns must have one entry per vector")
        all_ids = np.concatenate([old_ids, new_ids])
        order = np.argsort(all_ids, kind="stable")
        if np.any(np.diff(all_ids[order]) == 0):
            raise ValueError(f"duplicate {self.id_field} in insert")
        self._reserve(n)
        # `vectors` may be a CUDA tensor (the device-resident backfill): it stays on the device
        by_id = np.argsort(new_ids, kind="stable")
        if np.array_equal(by_id, np.arange(n)):
            self.index.insert(vectors, new_ids)
        else:
            import torch
            if isinstance(vectors, torch.Tensor):
                sorted_rows = vectors.reshape(n, self.index.dim)[torch.as_tensor(by_id, device=vectors.device)]
            else:
                sorted_rows = np.asarray(vectors, dtype=np.float32).reshape(n, self.index.dim)[by_id]
            self.index.insert(sorted_rows, new_ids[by_id])
        for key in set(self.columns) | set(columns):
            merged = list(self.columns.get(key, [None] * old_ids.size)) + list(columns.get(key, [None] * n))
            self.columns[key] = [merged[i] for i in order]
        ts = (np.asarray(list(call_started_at), dtype="datetime64[us]") if call_started_at is not None
              else np.full((n,), np.datetime64("NaT"), dtype="datetime64[us]"))
        self.call_started_at = np.concatenate([self.call_started_at, ts])[order]
        self.call_ids = np.concatenate([self.call_ids, np.asarray(list(columns["call_id"]), dtype=object)])[order]
        if call_tags:
            self.call_tags.update(call_tags)
        if self.tech_tokens is not None:
            merged_t = self.tech_tokens + toks
            self.tech_tokens = [merged_t[i] for i in order]
        ents = self._new_entities(int(old_ids.size), ents, n)
        if ents is not None:
            merged_e = self.entities + ents
            self.entities = [merged_e[i] for i in order]
        self._pos_of_id = None
        self.generation += 1

    def _drop_host_rows(self, keep: np.ndarray) -> None:
        """The host side of a removal: every per-row sequence loses the rows whose `keep` entry is false."""
        kept = np.flatnonzero(keep)
        for key, vals in self.columns.items():
            self.columns[key] = [vals[i] for i in kept]
        self.call_ids = self.call_ids[keep]
        self.call_started_at = self.call_started_at[keep]
        if self.tech_tokens is not None:
            self.tech_tokens = [self.tech_tokens[i] for i in kept]
        if getattr(self, "entities", None) is not None:
            self.entities = [self.entities[i] for i in kept]
        self._pos_of_id = None
        self.generation += 1   # row positions moved: the exact-token lane and the BM25 lane rebuild

    def delete(self, ids) -> int:
        """Remove the rows with these ids (absent ids are ignored) from the index, in place, and from the
        columns, call ids, timestamps, tech tokens and entities.  Returns the number of rows removed.  `call_tags`
        entries of calls that have no rows left may stay."""
        old_ids = np.asarray(self.columns.get(self.id_field, []), dtype=np.int64)
        keep = ~np.isin(old_ids, np.asarray(list(ids), dtype=np.int64))
        gone = int(keep.size - np.count_nonzero(keep))
        if gone == 0:
            return 0
        removed = self.index.remove(old_ids[~keep])
        if removed != gone:
            raise RuntimeError(f"{self.name}: the index removed {removed} rows where the columns hold {gone}")
        self._drop_host_rows(keep)
        return gone

    def delete_calls(self, call_ids) -> int:
        """Remove every row of these calls -- what `calls(call_id) ON DELETE CASCADE` does to the table
        (alembic/versions/0001_initial_schema.py:59,79,123).  Returns the number of rows removed."""
        wanted = set(call_ids)
        keep = np.fromiter((c not in wanted for c in self.call_ids), dtype=bool, count=len(self.call_ids))
        gone = int(keep.size - np.count_nonzero(keep))
        if gone == 0:
            return 0
        if self.index.compact(keep) != keep.size - gone:
            raise RuntimeError(f"{self.name}: the index and the columns disagree about the rows of the deleted calls")
        self._drop_host_rows(keep)
        return gone

    def sink(self, row_columns):
        """Backfill sink (embedding_pipeline.BackfillStore.update_embeddings -> HBM): an object whose
        `add(vectors, ids=...)` asks `row_columns(ids)` for the rows' SELECTed columns — a dict of column
        lists that may also carry "call_started_at", "tech_tokens" and "entities" (per-row lists of (label, value) pairs
        or {"label", "value"} dicts, the rows' chunk_entities / artifact_entities) — and inserts them here, so that the
        host-side columns, the filter masks, the exact-token lane and the index stay one table.  `vectors` may be
        host lists / arrays or a CUDA tensor (DeviceSinkStore)."""
        table = self

        class _Sink:
            def add(self, vectors, ids):
                cols = dict(row_columns(list(ids)))
                started = cols.pop("call_started_at", None)
                cols.setdefault(table.id_field, list(ids))
                table.insert(vectors, cols, call_started_at=started)

        return _Sink()

    # -- _build_filter_clause (retrieve.py:93-120) as a row mask --------------------------------
    def filter_mask(self, filters: Optional[RetrieveFilters], call_ids: Optional[Sequence[UUID]]
                    ) -> Optional[np.ndarray]:
        n = len(self)
        keep: Optional[np.ndarray] = None

        def land(cond: np.ndarray) -> None:
            nonlocal keep
            keep = cond if keep is None else (keep & cond)

        if filters:
            if filters.date_from:
                land(self.call_started_at >= np.datetime64(_naive_utc(filters.date_from), "us"))
            if filters.date_to:
                land(self.call_started_at <= np.datetime64(_naive_utc(filters.date_to), "us"))
            if call_ids is not None:
                wanted = set(call_ids)
                land(np.fromiter((c in wanted for c in self.call_ids), dtype=bool, count=n))
            if filters.call_tags:
                tags = set(filters.call_tags)
                ok_calls = {c for c, t in self.call_tags.items() if tags.intersection(t or ())}
                land(np.fromiter((c in ok_calls for c in self.call_ids), dtype=bool, count=n))
            if _has_attr_filters(filters):
                # row-level clauses: AND across clauses, OR inside one; a namespace this table lacks is
                # NULL and fails every clause over it
                from .filters import attr_clauses
                rows = [frozenset(attrs) for attrs in self._row_attrs()]
                for clause in attr_clauses(filters):
                    wanted_attrs = frozenset(clause)
                    land(np.fromiter((not wanted_attrs.isdisjoint(attrs) for attrs in rows), dtype=bool, count=n))
        return keep

    def _row_attrs(self):
        """Per row its attributes as (namespace, value) pairs in normal form: the `speaker` entry, the `kind` entry (where
        the table has the column) and the tracked entities."""
        from .filters import row_attributes
        return row_attributes(len(self), self.columns.get("speaker"), self.columns.get("kind"),
                              getattr(self, "entities", None))

    def _call_positions(self) -> Dict[Any, np.ndarray]:
        """call id -> the ascending positions of its rows, built in one host pass per (generation, length), the way
        `_positions` is cached."""
        key = (getattr(self, "generation", 0), len(self))
        memo = getattr(self, "_call_pos", None)
        if memo is None or memo[0] != key:
            by_call: Dict[Any, List[int]] = {}
            for i, c in enumerate(self.call_ids):
                by_call.setdefault(c, []).append(i)
            memo = self._call_pos = (key, {c: np.asarray(v, dtype=np.intp) for c, v in by_call.items()})
        return memo[1]

    def scoped_positions(self, filters: Optional[RetrieveFilters], call_ids: Optional[Sequence[UUID]],
                         limit: int) -> Optional[np.ndarray]:
        """np.flatnonzero(filter_mask(filters, call_ids)) for a call-scoped request, without a pass over all rows:
        the rows of the scoped calls come from the call -> positions map, the date and tag predicates are applied to
        those positions only.  None when the route does not apply: `filters` is falsy (filter_mask honours call_ids
        only under truthy filters), call_ids is None, the request carries an attribute clause (entity_filters, speakers,
        kinds), or the scoped calls together hold more than `limit` rows.  Host only."""
        if not filters or call_ids is None or _has_attr_filters(filters):
            return None   # (a row-level clause: the masked scan answers, same rows and score bits by construction)
        by_call = self._call_positions()
        parts = [by_call[c] for c in set(call_ids) if c in by_call]
        if sum(int(p.size) for p in parts) > int(limit):
            return None
        if filters.call_tags:
            tags = set(filters.call_tags)
            parts = [p for p in parts if tags.intersection(self.call_tags.get(self.call_ids[p[0]]) or ())]
        pos = np.sort(np.concatenate(parts)) if parts else np.empty((0,), dtype=np.intp)
        if filters.date_from:
            pos = pos[self.call_started_at[pos] >= np.datetime64(_naive_utc(filters.date_from), "us")]
        if filters.date_to:
            pos = pos[self.call_started_at[pos] <= np.datetime64(_naive_utc(filters.date_to), "us")]
        return pos

    # -- the same clause evaluated on the GPU (cadence_rag_amd.filters, crag_filter_masks_host) ----------
    def _device_columns(self, attr_name: str, build, close_old: bool = True):
        """The column set kept in `attr_name`, rebuilt by `build(device, generation)` on first use and again when
        `generation` or the length changed -- the way the exact-token and BM25 lanes follow the generation.  A kernel in
        flight may still read the old columns: the device is synchronised before they go.  close_old: the set owns an
        upload ring to close and feeds the masks, so the mask memo goes with it."""
        import torch
        cols = getattr(self, attr_name)
        if cols is None or cols.generation != self.generation or cols.n != len(self):
            if cols is not None:
                torch.cuda.synchronize(self.index.device)
                if close_old:
                    cols.close()
            if close_old:
                self._mask_memo = None
            cols = build(torch.device("cuda", self.index.device), self.generation)
            setattr(self, attr_name, cols)
        return cols

    def filter_columns(self):
        """The table's device filter columns (FilterColumns: call_started_at and the call number of every row in
        HBM, 12 bytes per row), built in one host pass per generation."""
        from .filters import FilterColumns
        return self._device_columns("_filter_cols", lambda device, generation: FilterColumns(
            self.call_started_at, self.call_ids, device=device, generation=generation))

    def attribute_columns(self):
        """The table's device attribute columns (filters.AttributeColumns: the rows' speaker, kind and entities as a CSR
        of dictionary ids in HBM, 8 bytes per row + 4 per attribute), built in one host pass per generation, like
        `filter_columns`.  Only a request with an attribute clause builds them."""
        from .filters import AttributeColumns
        return self._device_columns("_attr_cols", lambda device, generation: AttributeColumns(
            self._row_attrs(), device=device, generation=generation))

    def facet_columns(self):
        """The table's device facet columns (filters.FacetColumns: the attributes renumbered by (namespace, value) and
        stored as postings, 8 bytes per posting + 8 per attribute of HBM), built from `attribute_columns()` per
        generation.  Only a request that asks for facets builds them."""
        from .filters import FacetColumns
        return self._device_columns("_facet_cols", lambda device, generation: FacetColumns(
            self.attribute_columns(), device=device, generation=generation), close_old=False)

    def facets(self, batch: Sequence[Tuple[Optional[RetrieveFilters], Optional[Sequence[UUID]]]],
               namespaces: Sequence[str], top: int = 10) -> List[Dict[str, Any]]:
        """Facet counts for a batch of up to 64 (filters, call_ids) pairs -- the arguments of
        `filter_mask`: per query {"rows": the rows that pass its filters, "facets": {namespace: {"values": [{"value",
        "count"}, ...], "distinct": int}}} with the `top` values of each requested namespace ("speaker", "kind",
        "entity:LABEL", reported as given) by count descending, then value ascending; `distinct` is their number before
        the cut.  The masks (filter_masks_device) and the counts (crag_facet_counts_host) run on one stream with ONE
        synchronisation at the end; a batch in which no query filters anything passes no mask."""
        import torch

        from .filters import MAX_FACET_NAMESPACES, MAX_FACET_TOP, MAX_QUERIES
        batch = list(batch)
        names = list(dict.fromkeys(namespaces))
        if not 1 <= len(batch) <= MAX_QUERIES:
            raise ValueError(f"a facet batch holds 1 to {MAX_QUERIES} queries (got {len(batch)}): the caller splits it")
        if len(names) > MAX_FACET_NAMESPACES:
            raise ValueError(f"a facet request lists at most {MAX_FACET_NAMESPACES} namespaces (got {len(names)})")
        if not 1 <= int(top) <= MAX_FACET_TOP:
            raise ValueError(f"top must be in 1..{MAX_FACET_TOP}")
        fcols = self.facet_columns()
        stream = torch.cuda.current_stream(fcols.device)
        masks = None
        if any(self.filter_mask_applies(f, c) for f, c in batch):
            masks, _stride = self.filter_masks_device(batch, stream=stream.cuda_stream)
        out = fcols.counts(names, masks=masks, nq=len(batch), top=int(top), stream=stream.cuda_stream)
        stream.synchronize()
        return fcols.lists(names, *(t.cpu().numpy() for t in out))

    @staticmethod
    def filter_mask_applies(filters: Optional[RetrieveFilters], call_ids: Optional[Sequence[UUID]]) -> bool:
        """`filter_mask(filters, call_ids)` restricts something (it returns a mask, not None)."""
        return bool(filters) and bool(filters.date_from or filters.date_to or call_ids is not None or filters.call_tags
                                      or _has_attr_filters(filters))

    def filter_masks_device(self, batch: Sequence[Tuple[Optional[RetrieveFilters], Optional[Sequence[UUID]]]],
                            stream: Optional[int] = None):
        """Per-query masks for a batch of up to 64 (filters, call_ids) pairs -- the arguments of `filter_mask` --
        built by one kernel launch: (uint8 CUDA tensor [nq, stride], stride), what HybridSearcher.search(row_mask=,
        mask_stride=) and the lanes take.  An unfiltered query gets all ones up to len(self).  Enqueued on `stream`
        (default: torch's current stream) without a host synchronisation: a consumer on another stream orders itself
        behind it.  More than 64 queries: ValueError, the caller splits."""
        from .filters import compile_attr_predicates, compile_predicates, is_unfiltered
        batch = list(batch)
        if not batch:
            raise ValueError("filter_masks_device needs at least one query")
        cols = self.filter_columns()
        compiled = compile_predicates(cols, self.call_tags, batch)
        if not any(_has_attr_filters(f) for f, _ in batch):
            out = cols.masks(*compiled, stream=stream)
            return out, int(out.shape[1])
        # attribute clauses: their kernel runs in place behind the filter kernel on the same stream, or alone (no input
        # mask) when no query carries a call or date predicate
        acols = self.attribute_columns()
        attrs = compile_attr_predicates(acols, batch)
        if is_unfiltered(*compiled):
            out = acols.masks(attrs, stream=stream, nq=len(batch))
        else:
            out = cols.masks(*compiled, stream=stream)
            acols.masks(attrs, in_mask=out, in_stride=int(out.shape[1]), stride=int(out.shape[1]), out=out, stream=stream)
        return out, int(out.shape[1])

    def filter_mask_device(self, filters: Optional[RetrieveFilters], call_ids: Optional[Sequence[UUID]]):
        """`filter_mask` on the GPU: the packed mask as a uint8 CUDA tensor [ceil(n/32)*4] (== pack_mask(filter_mask(..))),
        or None exactly when `filter_mask` returns None.  No pass over the rows on the host.  The mask is COMPLETE on
        return (the producing stream is synchronised once), so the synchronous entries of the index, which run on a
        stream of their own, may read it; the lanes of one request ask for the same predicates eight times and get the
        same tensor (a one-entry memo per table, dropped with the generation).  `call_tags` that change reach the memo
        through `add` / `insert`, which bump the generation.  A request with row-level clauses (entity_filters, speakers,
        kinds) also runs the attribute kernel (crag_attr_masks_host); one without them never builds the attribute columns."""
        import torch

        if not self.filter_mask_applies(filters, call_ids):
            return None
        cols = self.filter_columns()
        key = (cols.generation, cols.n, filters.date_from, filters.date_to,
               None if call_ids is None else tuple(call_ids), tuple(filters.call_tags or ()))
        if _has_attr_filters(filters):
            key += (tuple((e.get("label"), e.get("value")) if isinstance(e, dict) else tuple(e)
                          for e in getattr(filters, "entity_filters", None) or ()),
                    tuple(getattr(filters, "speakers", None) or ()), tuple(getattr(filters, "kinds", None) or ()))
        if self._mask_memo is not None and self._mask_memo[0] == key:
            return self._mask_memo[1]
        mask = self.filter_masks_device([(filters, call_ids)])[0][0]   # one launch, or two with both kinds of predicate
        torch.cuda.current_stream(cols.device).synchronize()
        self._mask_memo = (key, mask)
        return mask

    def estimate_candidates(self, filters: Optional[RetrieveFilters], call_ids: Optional[Sequence[UUID]]) -> int:
        """COUNT(*) ... WHERE <filters> AND embedding IS NOT NULL (retrieve.py:303-323)."""
        return self.index.count_eligible(self.filter_mask_device(filters, call_ids))

    def fetch_dense(self, query_embedding, filters: Optional[RetrieveFilters],
                    call_ids: Optional[Sequence[UUID]], mode: str, limit: int,
                    select: Sequence[str], per_call: Optional[int] = None, mmr=None) -> List[Dict[str, Any]]:
        """ORDER BY embedding <=> q LIMIT :limit, rows as mappings with `select` columns + score.  per_call: at most
        that many rows of one call among them -- the best rows under the cap over the WHOLE table (the grouped search,
        crag_index_search_grouped_async, over the filter columns' call numbers), not a cut of the plain top-`limit`.
        mmr (cadence_rag_amd.mmr.MmrParams): the lane fetches mmr.fetch rows by the same route, picks `limit` of them by
        maximal marginal relevance on the GPU (DenseIndex.mmr: relevance = the row's cosine to the query, redundancy =
        its largest cosine to a row picked before) and returns them in pick order, `score` still the cosine."""
        del mode  # the HBM scan is always exact; `mode` only labels what pgvector would have done
        if len(self) == 0 or limit <= 0:
            return []
        q = _parse_vector(query_embedding)
        if mmr is not None:
            return self._fetch_dense_mmr(q, filters, call_ids, int(limit), select, per_call, mmr)
        if per_call:
            # (the listed-rows route below has no cap: every capped request takes the grouped search)
            ids, scores, _, counts = self._search_per_call(q, filters, call_ids, int(limit), int(per_call))
            return self._dense_rows(ids, scores, counts, select)
        rows: List[Dict[str, Any]] = []
        # the reference's "exact" dense mode (retrieve.py:277-287): a call-scoped request whose calls hold few rows reads
        # those rows only (crag_index_search_ids_async) -- the same rows and score bits as the masked scan below
        from ._native import CRAG_SUBSET_MAX_WIDTH
        cap = min(max(settings.embeddings_exact_scan_threshold, 0), CRAG_SUBSET_MAX_WIDTH)
        listed = self.scoped_positions(filters, call_ids, cap) if cap > 0 else None
        if listed is not None:
            if listed.size == 0:
                return []
            id_col = self.columns[self.id_field]
            ids, scores, counts = self.index.search_ids(q[None, :], [[int(id_col[i]) for i in listed]],
                                                        min(int(limit), _native_max_k()))
        else:
            ids, scores, counts = self.index.search(q[None, :], min(int(limit), _native_max_k()),
                                                    row_mask=self.filter_mask_device(filters, call_ids))
        pos_of = self._positions()
        for rid, sc in zip(ids[0, :counts[0]], scores[0, :counts[0]]):
            pos = pos_of[int(rid)]
            row = {name: self.columns[name][pos] for name in select}
            row["score"] = float(sc)
            rows.append(row)
        return rows

    def _fetch_dense_mmr(self, q: np.ndarray, filters, call_ids, limit: int, select: Sequence[str],
                         per_call: Optional[int], mmr) -> List[Dict[str, Any]]:
        """fetch_dense with MMR: mmr.fetch_for(limit) rows (a search returns at most CRAG_MAX_K) by the route the request
        takes without it -- the grouped search under a cap, the listed rows of a small call scope, else the masked
        search --, then `limit` picks among them.  The search's ids, scores and count stay on the device: the MMR call
        follows the search on the same stream and only the picks come back."""
        import torch

        from ._native import CRAG_MMR_MAX_WIDTH, CRAG_SUBSET_MAX_WIDTH
        ix = self.index
        limit = min(limit, CRAG_MMR_MAX_WIDTH)
        fetch = min(mmr.fetch_for(limit), _native_max_k())
        dev = torch.device("cuda", ix.device)
        stream = torch.cuda.current_stream(dev).cuda_stream
        d_q = torch.from_numpy(np.ascontiguousarray(q[None, :], dtype=np.float32)).to(dev)
        d_ids = torch.empty(1, fetch, dtype=torch.int64, device=dev)
        d_rel = torch.empty(1, fetch, dtype=torch.float32, device=dev)
        d_ct = torch.empty(1, dtype=torch.int32, device=dev)
        listed = None
        if not per_call:
            cap = min(max(settings.embeddings_exact_scan_threshold, 0), CRAG_SUBSET_MAX_WIDTH)
            listed = self.scoped_positions(filters, call_ids, cap) if cap > 0 else None
        if listed is not None:
            if listed.size == 0:
                return []
            id_col = self.columns[self.id_field]
            d_list = torch.tensor([[int(id_col[i]) for i in listed]], dtype=torch.int64, device=dev)
            d_n = torch.tensor([int(listed.size)], dtype=torch.int32, device=dev)
            ix.search_ids_async(d_q, d_list, d_n, fetch, d_ids, d_rel, d_ct, stream=stream)
        else:
            mask = self.filter_mask_device(filters, call_ids)   # (complete in memory on return; shared: stride 0)
            if per_call:
                cols = self.filter_columns()
                ix.search_grouped_async(d_q, fetch, cols.d_call_slot, cols.n_calls, int(per_call), d_ids, d_rel, d_ct,
                                        d_row_mask=mask, stream=stream)
            else:
                ix.search_async(d_q, fetch, d_ids, d_rel, d_ct, d_row_mask=mask, stream=stream)
        o_ids = torch.empty(1, limit, dtype=torch.int64, device=dev)
        o_rel = torch.empty(1, limit, dtype=torch.float32, device=dev)
        o_ct = torch.empty(1, dtype=torch.int32, device=dev)
        ix.mmr_async(d_ids, d_rel, d_ct, float(mmr.lam), limit, o_ids, o_rel, o_ct, stream=stream)
        return self._dense_rows(o_ids.cpu().numpy(), o_rel.cpu().numpy(), o_ct.cpu().numpy(), select)

    def _search_per_call(self, q: np.ndarray, filters, call_ids, limit: int, per_call: int):
        """The grouped search of one query under the request's filters: group = the row's call number."""
        cols = self.filter_columns()
        return self.index.search_grouped(q[None, :], min(int(limit), _native_max_k()), cols.d_call_slot, cols.n_calls,
                                         per_call, row_mask=self.filter_mask_device(filters, call_ids))

    def _dense_rows(self, ids, scores, counts, select: Sequence[str]) -> List[Dict[str, Any]]:
        pos_of = self._positions()
        rows: List[Dict[str, Any]] = []
        for rid, sc in zip(ids[0, :counts[0]], scores[0, :counts[0]]):
            pos = pos_of[int(rid)]
            row = {name: self.columns[name][pos] for name in select}
            row["score"] = float(sc)
            rows.append(row)
        return rows

    def shortlist_calls(self, query_embedding, filters: Optional[RetrieveFilters],
                        call_ids: Optional[Sequence[UUID]], n: int) -> List[Tuple[Any, int, float]]:
        """The call shortlist of the hierarchical strategy (APP_SPEC.md 9.2): the `n` calls whose best row scores
        highest under the request's filters, as [(call_id, id of that row, its score)], best first -- the grouped search
        with one row per call and k = n (at most CRAG_MAX_K calls)."""
        if len(self) == 0 or n <= 0:
            return []
        ids, scores, _, counts = self._search_per_call(_parse_vector(query_embedding), filters, call_ids, int(n), 1)
        pos_of = self._positions()
        return [(self.call_ids[pos_of[int(rid)]], int(rid), float(sc))
                for rid, sc in zip(ids[0, :counts[0]], scores[0, :counts[0]])]

    @classmethod
    def from_rows(cls, name: str, id_field: str, rows, *, select: Sequence[str], dim: Optional[int] = None,
                  call_tags: Optional[Dict[Any, Sequence[str]]] = None, batch: int = 65536,
                  device: Optional[int] = None, headroom: float = 0.25) -> Tuple["DenseTable", List[List[str]]]:
        """Startup loader: `rows` are the mappings of
            SELECT <select>, call_started_at, tech_tokens, embedding FROM <name>
            WHERE embedding IS NOT NULL ORDER BY <id_field>
        with `embedding` in any of pgvector's forms (text literal '[v,...]', binary send/recv bytes, or a
        sequence of floats).  A row may also carry "entities": its (label, value) pairs or {"label", "value"} dicts
        (the join to chunk_entities / artifact_entities), which the table keeps for the entity filters as it keeps
        "speaker" and "kind" among the SELECTed columns.  Returns the table and the per-row tech_tokens (for build_tech_lane).  Rows must
        come in ascending id order so that equal scores resolve to the lower id, as ORDER BY does.  The
        index is allocated with `headroom` spare capacity for the rows ingest / backfill add later (it
        also grows on demand, see `_reserve`)."""
        from . import vector_io
        rows = list(rows)
        d = dim or settings.embeddings_dim
        table = cls(name, id_field, dim=d, capacity=max(int(len(rows) * (1.0 + max(headroom, 0.0))) + 64, 1),
                    device=device)
        tokens: List[List[str]] = []
        last_id = None
        for lo in range(0, len(rows), batch):
            part = rows[lo:lo + batch]
            vecs = np.empty((len(part), d), dtype=np.float32)
            for i, row in enumerate(part):
                emb = row["embedding"]
                if isinstance(emb, str):
                    vecs[i] = vector_io.parse_vector(emb, d)
                elif isinstance(emb, (bytes, bytearray, memoryview)):
                    v = vector_io.from_binary(bytes(emb))
                    if v.size != d:
                        raise ValueError(f"expected {d} dimensions, not {v.size}")
                    vecs[i] = v
                else:
                    vecs[i] = np.asarray(emb, dtype=np.float32).reshape(d)
                rid = row[id_field]
                if last_id is not None and rid <= last_id:
                    raise ValueError(f"rows must be in ascending {id_field} order ({rid} after {last_id})")
                last_id = rid
                tokens.append(list(row.get("tech_tokens") or []))
            cols = {c: [row[c] for row in part] for c in select}
            if any("entities" in row for row in part):
                cols["entities"] = [row.get("entities") or [] for row in part]
            table.add(vecs, cols, call_started_at=[row.get("call_started_at") for row in part],
                      call_tags=call_tags if lo == 0 else None)
        return table, tokens

    def build_tech_lane(self, row_tokens: Optional[Sequence[Sequence[str]]] = None):
        """GPU exact-token lane over this table's rows (row i <-> position i, so filter masks are shared):
        the `tech_tokens text[]` column + ORDER BY call_started_at DESC, id ASC (retrieve.py:183-242).
        The table keeps the tokens from here on (rows added later bring theirs in `columns["tech_tokens"]`), and
        the lane remembers the table generation it was built for: GpuRetrieveBackend rebuilds a stale lane."""
        import torch

        from .fusion import TechTokenIndex
        if row_tokens is None:
            row_tokens = self.tech_tokens
            if row_tokens is None:
                raise ValueError("this table does not track tech_tokens yet: pass row_tokens")
        if len(row_tokens) != len(self):
            raise ValueError("row_tokens must have one entry per table row")
        self.tech_tokens = [list(t or []) for t in row_tokens]
        lane = TechTokenIndex(self.tech_tokens, np.asarray(self.columns[self.id_field], dtype=np.int64),
                              self.call_started_at, torch.device("cuda", self.index.device))
        lane.table_generation = self.generation
        return lane

    def build_bm25_lane(self, text_column: str, positions: bool = False):
        """GPU BM25 lane (cadence_rag_amd.bm25.Bm25Index, non-parity with pg_search) over this table's
        `text_column` -- "text" for chunks, "content" for artifact_chunks (retrieve.py:141,173).  Row i <-> position i,
        so `filter_mask` serves this lane as it serves the other two.  The lane remembers the column and the table
        generation it was built for: `sync_bm25_lane` brings a stale one up to date.  positions: also index the token
        positions, which the phrase clauses of the query syntax need (settings.bm25_query_syntax)."""
        import torch

        from .bm25 import Bm25Index
        if text_column not in self.columns and len(self):
            raise ValueError(f"{self.name} has no column {text_column!r}")
        lane = Bm25Index(self.columns.get(text_column, []), np.asarray(self.columns.get(self.id_field, []), dtype=np.int64),
                         torch.device("cuda", self.index.device), positions=positions)
        lane.text_column = text_column
        lane.table_generation = self.generation
        return lane

    def sync_bm25_lane(self, lane):
        """The lane for the table as it is now: unchanged when it is current, grown with `extend` (only the new rows
        are tokenised) when rows were appended behind the ones it holds, rebuilt when rows moved (`insert`) or left
        (`delete`: a table that shrank never passes for one that grew, the lane then holds more rows than the table
        or ids the table no longer has at those positions)."""
        if getattr(lane, "table_generation", None) == self.generation and len(lane) == len(self):
            return lane
        ids = np.asarray(self.columns.get(self.id_field, []), dtype=np.int64)
        held = len(lane)
        if held <= ids.size and np.array_equal(ids[:held], lane.ids):
            if held < ids.size:
                lane.extend(self.columns[lane.text_column][held:], ids[held:])
            lane.table_generation = self.generation
            return lane
        return self.build_bm25_lane(lane.text_column, positions=bool(getattr(lane, "positions", False)))

    def build_ngram_lane(self, text_column: str):
        """GPU character-trigram lane (cadence_rag_amd.ngram.NgramIndex: the reference's `pdb.ngram(3,3)` alias of the
        column, a self-defined rule) over this table's `text_column`, its postings built on the device.  Row i <->
        position i; the lane remembers the column and the table generation, as the BM25 lane does."""
        import torch

        from .ngram import NgramIndex
        if text_column not in self.columns and len(self):
            raise ValueError(f"{self.name} has no column {text_column!r}")
        lane = NgramIndex(self.columns.get(text_column, []), np.asarray(self.columns.get(self.id_field, []), dtype=np.int64),
                          torch.device("cuda", self.index.device))
        lane.text_column = text_column
        lane.table_generation = self.generation
        return lane

    def sync_ngram_lane(self, lane):
        """`sync_bm25_lane` for the trigram lane: unchanged when current, grown with `extend` when rows were appended
        behind the ones it holds, rebuilt when rows moved or left."""
        if getattr(lane, "table_generation", None) == self.generation and len(lane) == len(self):
            return lane
        ids = np.asarray(self.columns.get(self.id_field, []), dtype=np.int64)
        held = len(lane)
        if held <= ids.size and np.array_equal(ids[:held], lane.ids):
            if held < ids.size:
                lane.extend(self.columns[lane.text_column][held:], ids[held:])
            lane.table_generation = self.generation
            return lane
        return self.build_ngram_lane(lane.text_column)

    def dedupe(self, ids, threshold: float) -> List[Tuple[Optional[int], Optional[float]]]:
        """Greedy near-duplicate suppression of one ranked list of row ids (best first, at most 256) over the stored
        vectors (DenseIndex.dedupe): per input id (slot of the kept, higher-ranked id that is at least `threshold`
        similar, that cosine), or (None, None) for an id that stays.  Ids without a stored vector always stay."""
        ids = [int(v) for v in ids]
        if not ids or len(self) == 0:
            return [(None, None)] * len(ids)
        _, dup_of, sim = self.index.dedupe(np.asarray(ids, dtype=np.int64), float(threshold))
        return [(None, None) if d < 0 else (int(d), float(c)) for d, c in zip(dup_of, sim)]

    def _positions(self) -> Dict[int, int]:
        if getattr(self, "_pos_of_id", None) is None:
            self._pos_of_id = {int(v): i for i, v in enumerate(self.columns[self.id_field])}
        return self._pos_of_id


def _native_max_k() -> int:
    from ._native import CRAG_MAX_K
    return CRAG_MAX_K


def _naive_utc(dt: datetime) -> datetime:
    if dt.tzinfo is not None:
        from datetime import timezone
        return dt.astimezone(timezone.utc).replace(tzinfo=None)
    return dt


CHUNK_SELECT = ("chunk_id", "call_id", "speaker", "start_ts_ms", "end_ts_ms", "text")
ARTIFACT_SELECT = ("artifact_chunk_id", "artifact_id", "call_id", "kind", "content")


def _dense_per_call_cap() -> int:
    """Settings.dense_per_call_cap as the grouped search takes it: 0 (off) .. CRAG_GROUP_MAX_PER."""
    from ._native import CRAG_GROUP_MAX_PER
    return min(max(int(settings.dense_per_call_cap or 0), 0), CRAG_GROUP_MAX_PER)


def _dense_mmr():
    """Settings.dense_mmr_lambda / dense_mmr_fetch as the dense lanes take them: None when the knob is off (1.0 or more:
    the plain ranking, nothing is launched), else the MmrParams with lambda clamped to [0, 1]."""
    from .mmr import MmrParams
    lam = float(settings.dense_mmr_lambda)
    if not lam < 1.0:   # (NaN: off)
        return None
    return MmrParams(lam=max(lam, 0.0), fetch=max(int(settings.dense_mmr_fetch or 0), 0))


def _estimate_dense_candidates(table: DenseTable, table_name: str, filters: Optional[RetrieveFilters],
                               call_ids: Optional[Sequence[UUID]]) -> int:
    del table_name
    return table.estimate_candidates(filters, call_ids)


def _fetch_chunks_dense(table: DenseTable, query_embedding, filters: Optional[RetrieveFilters],
                        call_ids: Optional[Sequence[UUID]], mode: str, limit: int) -> List[Dict[str, Any]]:
    """Same signature as the reference with the SQL connection replaced by the chunks DenseTable;
    rows: {chunk_id, call_id, speaker, start_ts_ms, end_ts_ms, text, score}, best first."""
    return table.fetch_dense(query_embedding, filters, call_ids, mode, limit, CHUNK_SELECT)


def _fetch_artifacts_dense(table: DenseTable, query_embedding, filters: Optional[RetrieveFilters],
                           call_ids: Optional[Sequence[UUID]], mode: str, limit: int) -> List[Dict[str, Any]]:
    """rows: {artifact_chunk_id, artifact_id, call_id, kind, content, score}, best first."""
    return table.fetch_dense(query_embedding, filters, call_ids, mode, limit, ARTIFACT_SELECT)


# ------------------------------------------------------------------------------------------------
# /retrieve entry point (S9): the orchestration of /root/reference/app/retrieve.py:392-688 with the
# SQL connection replaced by a backend object.  Lane order, RRF, ids_only ordering, evidence packing,
# budget clipping and every `notes.retrieval` / `debug` key follow the reference; goldens captured
# from the reference's own retrieve_evidence (tests/golden/reference_retrieve_evidence.json) pin it.
# ------------------------------------------------------------------------------------------------
DEFAULT_CHUNK_BM25_TOPK = 50
DEFAULT_ARTIFACT_CHUNK_BM25_TOPK = 10
DEFAULT_TECH_TOPK = 50
DEFAULT_MAX_ARTIFACTS = 2
DEFAULT_MAX_QUOTES_PER_CALL = 2
DEFAULT_SNIPPET_CHARS = 800


@dataclass
class Budget:
    """app/schemas.py:71-73."""
    max_evidence_items: int = 8
    max_total_chars: int = 6000

    def model_dump(self) -> Dict[str, int]:
        return {"max_evidence_items": self.max_evidence_items, "max_total_chars": self.max_total_chars}


@dataclass
class RetrieveRequest:
    """app/schemas.py:85-93."""
    query: str
    intent: str = "auto"
    filters: Optional[RetrieveFilters] = None
    budget: Optional[Budget] = None
    return_style: str = "evidence_pack_json"
    debug: bool = False
    # facet counts: the namespaces ("speaker", "kind", "entity:LABEL") to count over the rows that pass
    # `filters`, and how many values of each to list; None or [] asks for none and changes nothing
    facets: Optional[List[str]] = None
    facet_top: int = 10

    def __post_init__(self) -> None:
        from .filters import MAX_FACET_NAMESPACES, MAX_FACET_TOP
        if self.facets is not None and len(self.facets) > MAX_FACET_NAMESPACES:
            raise ValueError(f"facets lists at most {MAX_FACET_NAMESPACES} namespaces (got {len(self.facets)})")
        if not 1 <= int(self.facet_top) <= MAX_FACET_TOP:
            raise ValueError(f"facet_top must be in 1..{MAX_FACET_TOP} (got {self.facet_top})")


def _build_debug_lane(rows: Sequence[Dict[str, Any]], id_field: str) -> List[Dict[str, Any]]:
    """retrieve.py:32-41."""
    return [{id_field: row[id_field], "rank": rank, "score": row.get("score")}
            for rank, row in enumerate(rows, start=1)]


class RetrieveBackend:
    """What retrieve_evidence needs from storage: one method per SQL helper of the reference
    (retrieve.py:46-389), same arguments minus the connection.  Subclass or duck-type."""

    def resolve_call_ids(self, filters): return None
    def fetch_chunks_bm25(self, query, filters, call_ids, limit): return []
    def fetch_artifacts_bm25(self, query, filters, call_ids, limit): return []
    # the character-trigram field of the lexical lanes: None = this backend has no such lane (it then does not appear
    # anywhere in the response), a list = the lane ran
    def fetch_chunks_ngram(self, query, filters, call_ids, limit): return None
    def fetch_artifacts_ngram(self, query, filters, call_ids, limit): return None
    def fetch_chunks_tech(self, tokens, filters, call_ids, limit): return []
    def fetch_artifacts_tech(self, tokens, filters, call_ids, limit): return []
    def estimate_dense_candidates(self, table_name, filters, call_ids): return 0
    def fetch_chunks_dense(self, query_embedding, filters, call_ids, mode, limit): return []
    def fetch_artifacts_dense(self, query_embedding, filters, call_ids, mode, limit): return []

    def dedupe(self, table_name, ids, threshold):
        """Near-duplicate suppression of one side's fused ids (best first): per id (slot of the kept id that suppresses
        it, their cosine) or (None, None).  A backend without vectors drops nothing."""
        return [(None, None)] * len(ids)

    def snippet_windows(self, table_name, query, ids):
        """Where the snippet of every listed row should begin (settings.snippet_best): per id the pair
        (start, last) of token positions in the row's body column -- start < 0: no query word found -- or None when
        this backend cannot place snippets on that table: every row then keeps the head clip."""
        return None

    def facets(self, table_name, filters, call_ids, namespaces, top):
        """Facet counts of one table over the rows that pass the request's filters: {"rows": int, "facets": {namespace:
        {"values": [{"value", "count"}], "distinct": int}}}.  A backend without attributes has none: {}."""
        return {}


class GpuRetrieveBackend(RetrieveBackend):
    """Dense lanes from the HBM-resident DenseTables, exact-token lanes from GPU TechTokenIndex objects
    (cadence_rag_amd.fusion) when attached.  BM25 lanes: `bm25_chunks` / `bm25_artifacts` are either callables
    (query, filters, call_ids, limit) -> rows -- pg_search's own rows as an input, as they are to _rrf_merge -- or
    native lanes (cadence_rag_amd.bm25.Bm25Index from DenseTable.build_bm25_lane: a self-defined BM25, not parity
    with pg_search, whose arithmetic is not in the reference repository).  Trigram lanes, off unless given:
    `ngram_chunks` / `ngram_artifacts` are callables of the same shape or native lanes (cadence_rag_amd.ngram.NgramIndex
    from DenseTable.build_ngram_lane); a side with one adds the lane `bm25_ngram` behind `bm25`."""

    def __init__(self, chunks: DenseTable, artifact_chunks: DenseTable, *, calls: Sequence[Dict[str, Any]] = (),
                 bm25_chunks=None, bm25_artifacts=None, tech_chunks=None, tech_artifacts=None,
                 ngram_chunks=None, ngram_artifacts=None) -> None:
        self.tables = {"chunks": chunks, "artifact_chunks": artifact_chunks}
        self.calls = list(calls)
        self._bm25 = {"chunks": bm25_chunks, "artifact_chunks": bm25_artifacts}
        self._ngram = {"chunks": ngram_chunks, "artifact_chunks": ngram_artifacts}
        self._tech = {"chunks": tech_chunks, "artifact_chunks": tech_artifacts}

    def resolve_call_ids(self, filters):
        return _resolve_call_ids(self.calls, filters)

    @staticmethod
    def _lane_mask(table, lane, filters, call_ids):
        """The request's filters as the packed device mask of a lane over `table`: a DenseTable evaluates them on the GPU
        (filter_mask_device); a duck-typed table that brings only the host form `filter_mask` has it packed and
        uploaded."""
        on_device = getattr(table, "filter_mask_device", None)
        if on_device is not None:
            return on_device(filters, call_ids)
        import torch
        mask = table.filter_mask(filters, call_ids)
        return None if mask is None else torch.from_numpy(DenseIndex.pack_mask(mask)).to(lane.device)

    def _parsed_query(self, query):
        """The query in the clause syntax, or None when it is over the syntax's limits: the lanes then read the raw
        string as a bag of tokens.  Logged once per request: the lanes of one request ask with the same string."""
        from .bm25 import QuerySyntaxError, parse_query
        try:
            # (the keyword only when the setting is on: prefix and fuzzy items)
            return parse_query(query, expand=True) if settings.bm25_query_expand else parse_query(query)
        except QuerySyntaxError as exc:
            if getattr(self, "_syntax_logged", None) != query:
                self._syntax_logged = query
                _log.warning("BM25 query syntax: %s; the query is read as a bag of tokens", exc)
            return None

    def _bm25_rows(self, name, select, query, filters, call_ids, limit, field="bm25"):
        """retrieve.py:123-180: the SELECTed columns + `score`, best first.  field: "bm25", the word lane, or "ngram",
        the trigram lane (same rows, same limit, same mask; None when the side has no such lane)."""
        lanes, sync = (self._bm25, "sync_bm25_lane") if field == "bm25" else (self._ngram, "sync_ngram_lane")
        fn, table = lanes[name], self.tables[name]
        if fn is None:
            return [] if field == "bm25" else None
        # the clause syntax (settings.bm25_query_syntax): the word lane applies the clauses, the trigram
        # lane is given the non-excluded items' text.  A query over the syntax's limits is read as a bag, as without it
        parsed = self._parsed_query(query) if settings.bm25_query_syntax else None
        if parsed is not None and field == "ngram":
            query = parsed.text
        if callable(fn):
            return list(fn(query, filters, call_ids, limit))
        if len(table) == 0 or int(limit) <= 0:
            return []
        lane = lanes[name] = getattr(table, sync)(fn)
        d_mask = self._lane_mask(table, lane, filters, call_ids)
        search = lane.search_query if parsed is not None and field == "bm25" else lane.search
        # (a duck-typed lane's search_query may not know the keyword: it is passed only when the setting is on)
        more = {"expand": True} if parsed is not None and field == "bm25" and settings.bm25_query_expand else {}
        ids, scores, counts = search([query], min(int(limit), _native_max_k()), row_mask=d_mask, mask_stride=0, **more)
        n = int(counts[0])
        pos_of = table._positions()
        out = []
        for rid, sc in zip(ids[0, :n].tolist(), scores[0, :n].tolist()):
            pos = pos_of[int(rid)]
            row = {col: table.columns[col][pos] for col in select}
            row["score"] = float(sc)
            out.append(row)
        return out

    def fetch_chunks_bm25(self, query, filters, call_ids, limit):
        return self._bm25_rows("chunks", CHUNK_SELECT, query, filters, call_ids, limit)

    def fetch_artifacts_bm25(self, query, filters, call_ids, limit):
        return self._bm25_rows("artifact_chunks", ARTIFACT_SELECT, query, filters, call_ids, limit)

    def fetch_chunks_ngram(self, query, filters, call_ids, limit):
        return self._bm25_rows("chunks", CHUNK_SELECT, query, filters, call_ids, limit, field="ngram")

    def fetch_artifacts_ngram(self, query, filters, call_ids, limit):
        return self._bm25_rows("artifact_chunks", ARTIFACT_SELECT, query, filters, call_ids, limit, field="ngram")

    def _tech_rows(self, name, select, tokens, filters, call_ids, limit):
        lane, table = self._tech[name], self.tables[name]
        if not tokens or lane is None or len(table) == 0:
            return []
        if getattr(lane, "table_generation", table.generation) != table.generation or lane.n != len(table):
            # rows were appended or moved since the lane was built: its row positions (and with them every packed
            # mask bit) no longer mean the table's rows
            if table.tech_tokens is None or len(table.tech_tokens) != len(table):
                raise RuntimeError(f"the exact-token lane of {name} is stale (table generation {table.generation}) "
                                   "and the table does not track tech_tokens: rebuild it with build_tech_lane")
            lane = self._tech[name] = table.build_tech_lane()
        d_mask = self._lane_mask(table, lane, filters, call_ids)
        ids, counts = lane.search([list(tokens)], int(limit), row_mask=d_mask, mask_stride=0)
        pos_of = table._positions()
        out = []
        for rid in ids[0, : int(counts[0])].tolist():
            pos = pos_of[int(rid)]
            out.append({col: table.columns[col][pos] for col in select})
        return out

    def fetch_chunks_tech(self, tokens, filters, call_ids, limit):
        return self._tech_rows("chunks", CHUNK_SELECT, tokens, filters, call_ids, limit)

    def fetch_artifacts_tech(self, tokens, filters, call_ids, limit):
        return self._tech_rows("artifact_chunks", ARTIFACT_SELECT, tokens, filters, call_ids, limit)

    def estimate_dense_candidates(self, table_name, filters, call_ids):
        return _estimate_dense_candidates(self.tables[table_name], table_name, filters, call_ids)

    def fetch_chunks_dense(self, query_embedding, filters, call_ids, mode, limit):
        cap = _dense_per_call_cap()   # (the artifact side has no per-call quota in _pack: it stays uncapped)
        mmr = _dense_mmr()
        if mmr is not None:
            return self.tables["chunks"].fetch_dense(query_embedding, filters, call_ids, mode, limit, CHUNK_SELECT,
                                                     per_call=cap or None, mmr=mmr)
        if cap:
            return self.tables["chunks"].fetch_dense(query_embedding, filters, call_ids, mode, limit, CHUNK_SELECT,
                                                     per_call=cap)
        return _fetch_chunks_dense(self.tables["chunks"], query_embedding, filters, call_ids, mode, limit)

    def fetch_artifacts_dense(self, query_embedding, filters, call_ids, mode, limit):
        mmr = _dense_mmr()
        if mmr is not None:
            return self.tables["artifact_chunks"].fetch_dense(query_embedding, filters, call_ids, mode, limit,
                                                              ARTIFACT_SELECT, mmr=mmr)
        return _fetch_artifacts_dense(self.tables["artifact_chunks"], query_embedding, filters, call_ids, mode, limit)

    def facets(self, table_name, filters, call_ids, namespaces, top):
        return self.tables[table_name].facets([(filters, call_ids)], namespaces, top)[0]

    def snippet_windows(self, table_name, query, ids):
        """From the native word lane of the table when it was built with positions: one launch for all the rows
        (Bm25Index.snippet_windows, crag_bm25_snippets_host).  None for a callable lane, a lane without positions or
        rows the lane does not hold."""
        lane, table = self._bm25[table_name], self.tables[table_name]
        if lane is None or callable(lane) or not getattr(lane, "positions", False) or not ids or len(table) == 0:
            return None
        lane = self._bm25[table_name] = table.sync_bm25_lane(lane)
        try:
            start, last, _, _ = lane.snippet_windows([query], [list(ids)], int(settings.snippet_window_tokens))
        except ValueError as exc:
            _log.warning("snippet windows of %s: %s; the snippets are head clips", table_name, exc)
            return None
        return list(zip(start.tolist(), last.tolist()))

    def dedupe(self, table_name, ids, threshold):
        return self.tables[table_name].dedupe(ids, threshold)


_backend: Optional[RetrieveBackend] = None


def set_backend(backend: Optional[RetrieveBackend]) -> None:
    """Register the process-wide backend (the counterpart of the reference's module-level `engine`)."""
    global _backend
    _backend = backend


@dataclass(frozen=True)
class _Side:
    """One of the two evidence tables as /retrieve sees it: which lanes feed it, how one of its rows becomes
    an evidence item and which caps apply.  The response of /root/reference/app/retrieve.py:392-688 is a
    function of these two records and the request; tests/golden/reference_retrieve_evidence.json pins it."""
    table: str          # backend table name, also the key inside notes/debug dictionaries
    out: str            # response list ("artifacts" / "quotes") and debug.lanes key
    debug_key: str
    id_field: str
    tag: str            # ids_only prefix
    rank: int           # ids_only tie order: lower first
    letter: str         # evidence_id prefix
    body: str           # column the snippet is cut from
    carry: Tuple[str, ...]   # columns copied into the item, in response order
    bm25_topk: int
    dense_topk: int
    list_cap: Optional[int]  # at most this many items of this kind
    per_call: Optional[int]  # at most this many per call_id


_SIDES = (
    _Side("artifact_chunks", "artifacts", "artifacts", "artifact_chunk_id", "artifact_chunk", 0, "A", "content",
          ("artifact_id", "artifact_chunk_id", "kind"), DEFAULT_ARTIFACT_CHUNK_BM25_TOPK,
          DEFAULT_DENSE_ARTIFACT_CHUNK_TOPK, DEFAULT_MAX_ARTIFACTS, None),
    _Side("chunks", "quotes", "chunks", "chunk_id", "chunk", 1, "Q", "text",
          ("chunk_id", "speaker", "start_ts_ms", "end_ts_ms"), DEFAULT_CHUNK_BM25_TOPK,
          DEFAULT_DENSE_CHUNK_TOPK, None, DEFAULT_MAX_QUOTES_PER_CALL),
)
_BY_TABLE = {s.table: s for s in _SIDES}
# the backend is queried chunks first (the reference's statement order; the replay backend records it)
_QUERY_ORDER = (_BY_TABLE["chunks"], _BY_TABLE["artifact_chunks"])


class _Purse:
    """The request budget while the evidence pack is being filled."""

    def __init__(self, budget: Budget) -> None:
        self.items = budget.max_evidence_items
        self.chars = budget.max_total_chars

    @property
    def spent(self) -> bool:
        return self.items <= 0 or self.chars <= 0


def _pack(ranked, side: _Side, purse: _Purse, item_cap: Optional[int],
          windows: Optional[Dict[Any, Tuple[int, int]]] = None) -> List[Dict[str, Any]]:
    """Ranked rows of one side -> evidence items, best first, until the purse or the side's caps run out.
    A row over its call's quota is passed over without ending the walk.  windows: row id -> (start, last), the token
    window its snippet is cut around (settings.snippet_best); a row without one gets the head clip."""
    out: List[Dict[str, Any]] = []
    used_by_call: Dict[str, int] = {}
    for row, lanes, _ in ranked:
        if purse.spent or (item_cap is not None and len(out) >= item_cap):
            break
        call = str(row["call_id"])
        if side.per_call is not None:
            if used_by_call.get(call, 0) >= side.per_call:
                continue
            used_by_call[call] = used_by_call.get(call, 0) + 1
        at = windows.get(row[side.id_field]) if windows else None
        if at is None:
            snippet = _clip(row[side.body], min(DEFAULT_SNIPPET_CHARS, purse.chars))
        else:
            snippet = cut_snippet(row[side.body], at[0], at[1], min(DEFAULT_SNIPPET_CHARS, purse.chars))
        purse.chars -= len(snippet)
        purse.items -= 1
        item = {"evidence_id": f"{side.letter}-{row[side.id_field]}", "call_id": call}
        item.update((col, row[col]) for col in side.carry)
        item["snippet"] = snippet
        item["why_relevant"] = " + ".join(sorted(lanes))
        out.append(item)
    return out


class _DenseState:
    """What the dense lane contributed to one request (all of it is echoed in notes / debug)."""

    def __init__(self) -> None:
        self.on = False
        self.model_id: Optional[str] = None
        self.error: Optional[str] = None
        self.literal: Optional[str] = None
        self.mode: Dict[str, Optional[str]] = {s.table: None for s in _QUERY_ORDER}
        self.candidates: Dict[str, int] = {s.table: 0 for s in _QUERY_ORDER}

    def embed(self, query: str) -> None:
        from . import embeddings as _emb
        self.on = _emb.embeddings_enabled()
        if not self.on:
            return
        try:  # fail-open: a broken encoder turns the lane off for this request and is reported
            res = _emb.embed_texts([query])
        except _emb.EmbeddingClientError as exc:
            self.on, self.error = False, str(exc)
            return
        self.model_id, self.literal = res.model, _vector_literal(res.vectors[0])

    @property
    def planner(self) -> str:
        if not self.on:
            return "lexical_only"
        return "ann" if "ann" in self.mode.values() else "exact"

    def topk(self, side: _Side) -> int:
        return side.dense_topk if self.on else 0


class _RerankState:
    """What the reranker did to one request (echoed in notes when reranking is configured)."""

    def __init__(self) -> None:
        self.on = False
        self.model_id: Optional[str] = None
        self.error: Optional[str] = None
        self.scored: Optional[int] = None

    def apply(self, query: str, fused: Dict[str, List[Tuple[Dict[str, Any], Any, float]]]):
        """RRF -> rerank top N -> top M, per side: the first rerank_topn_in fused rows of each side are scored in ONE
        call (their full body column, both sides behind one shared query prefix), reordered by score (ties keep the
        RRF order) and cut to rerank_topm_out; the score replaces the RRF score.  Fail-open like the dense lane: on
        RerankClientError the fused lists come back as they are and the error is reported."""
        from . import reranker as _rr
        self.on = _rr.rerank_enabled()
        if not self.on:
            return fused
        n_in, m_out = max(settings.rerank_topn_in, 0), max(settings.rerank_topm_out, 0)
        heads = {s.table: list(fused[s.table][:n_in]) for s in _SIDES}
        docs = [str(row[s.body] or "") for s in _SIDES for row, _, _ in heads[s.table]]
        if not docs:
            return fused
        try:
            res = _rr.rerank_texts(query, docs)
        except _rr.RerankClientError as exc:
            self.error = str(exc)
            return fused
        self.model_id, self.scored = res.model, len(docs)
        out = dict(fused)
        at = 0
        for s in _SIDES:
            rows = heads[s.table]
            scores = res.scores[at:at + len(rows)]
            at += len(rows)
            keep = sorted(range(len(rows)), key=lambda i: (-scores[i], i))[:m_out]
            out[s.table] = [(rows[i][0], rows[i][1], scores[i]) for i in keep]
        return out


DEDUPE_MAX_ROWS = 256   # fused rows of a side that are examined (CRAG_DEDUPE_MAX_WIDTH); later rows pass through


class _DedupeState:
    """What near-duplicate suppression did to one request (echoed in notes / debug when the knob is on)."""

    def __init__(self) -> None:
        self.cosine = float(settings.evidence_dedupe_cosine or 0.0)
        self.on = self.cosine != 0.0
        self.dropped: Dict[str, int] = {s.table: 0 for s in _QUERY_ORDER}
        self.pairs: Dict[str, List[Dict[str, Any]]] = {s.debug_key: [] for s in _QUERY_ORDER}

    def apply(self, be: "RetrieveBackend", fused: Dict[str, List[Tuple[Dict[str, Any], Any, float]]]):
        """Per side, in front of the reranker: a fused row goes when a kept, higher-ranked row of its side is at least
        `cosine` similar to it -- the copy RRF ranked higher survives and duplicates cost no reranker slots."""
        if not self.on:
            return fused
        out = dict(fused)
        for s in _QUERY_ORDER:
            rows = fused[s.table]
            ids = [row[s.id_field] for row, _, _ in rows[:DEDUPE_MAX_ROWS]]
            if not ids:
                continue
            verdict = be.dedupe(s.table, ids, self.cosine)
            kept = []
            for slot, (dup_of, cos) in enumerate(verdict):
                if dup_of is None:
                    kept.append(rows[slot])
                else:
                    self.pairs[s.debug_key].append({"dropped": ids[slot], "kept": ids[dup_of], "cosine": cos})
            self.dropped[s.table] = len(ids) - len(kept)
            out[s.table] = kept + list(rows[len(ids):])
        return out


def _gather_lanes(be: "RetrieveBackend", query: str, tokens: List[str], filters, dense: _DenseState
                  ) -> Dict[str, Dict[str, Sequence[Dict[str, Any]]]]:
    """table -> {lane name -> rows}, lanes in fusion order (bm25, [bm25_ngram,] tech_tokens, dense): the trigram lane
    exists only where the backend returns a list for it."""
    call_ids = be.resolve_call_ids(filters)
    ngram = {"chunks": getattr(be, "fetch_chunks_ngram", None), "artifact_chunks": getattr(be, "fetch_artifacts_ngram", None)}
    fetch = {"chunks": (be.fetch_chunks_bm25, be.fetch_chunks_tech, be.fetch_chunks_dense),
             "artifact_chunks": (be.fetch_artifacts_bm25, be.fetch_artifacts_tech, be.fetch_artifacts_dense)}
    lanes: Dict[str, Dict[str, Sequence[Dict[str, Any]]]] = {s.table: {} for s in _QUERY_ORDER}
    for s in _QUERY_ORDER:
        lanes[s.table]["bm25"] = fetch[s.table][0](query, filters, call_ids, s.bm25_topk)
        rows = ngram[s.table](query, filters, call_ids, s.bm25_topk) if ngram[s.table] is not None else None
        if rows is not None:
            lanes[s.table]["bm25_ngram"] = rows
    for s in _QUERY_ORDER:
        lanes[s.table]["tech_tokens"] = fetch[s.table][1](tokens, filters, call_ids, DEFAULT_TECH_TOPK)
    if dense.on and dense.literal is not None:
        for s in _QUERY_ORDER:
            dense.candidates[s.table] = be.estimate_dense_candidates(s.table, filters, call_ids)
        for s in _QUERY_ORDER:
            dense.mode[s.table] = _choose_dense_mode(dense.candidates[s.table], filters, call_ids)
    if dense.on:
        for s in _QUERY_ORDER:
            lanes[s.table]["dense"] = (fetch[s.table][2](dense.literal, filters, call_ids, dense.mode[s.table],
                                                         s.dense_topk) if dense.literal is not None else [])
    return lanes


def _debug_section(lanes, dense: _DenseState) -> Dict[str, Any]:
    chunks, artifacts = _BY_TABLE["chunks"], _BY_TABLE["artifact_chunks"]
    return {
        "lanes": {s.debug_key: {name: _build_debug_lane(rows, s.id_field) for name, rows in lanes[s.table].items()}
                  for s in _QUERY_ORDER},
        "limits": {"bm25_chunk_topk": chunks.bm25_topk, "bm25_artifact_chunk_topk": artifacts.bm25_topk,
                   "tech_token_topk": DEFAULT_TECH_TOPK, "dense_chunk_topk": dense.topk(chunks),
                   "dense_artifact_chunk_topk": dense.topk(artifacts)},
        "dense": {"enabled": dense.on, "model_id": dense.model_id, "error": dense.error,
                  "modes": dict(dense.mode), "candidate_rows": dict(dense.candidates)},
    }


def _retrieval_notes(tokens: List[str], dense: _DenseState, rerank: Optional[_RerankState] = None,
                     dedupe: Optional[_DedupeState] = None, lanes=None) -> Dict[str, Any]:
    chunks, artifacts = _BY_TABLE["chunks"], _BY_TABLE["artifact_chunks"]
    notes = {
        "planner": dense.planner,
        "dense_topk": max(dense.topk(chunks), dense.topk(artifacts)),
        "lex_topk": chunks.bm25_topk,
        "artifact_chunk_lex_topk": artifacts.bm25_topk,
        "reranked_from": None,
        "bm25_chunk_topk": chunks.bm25_topk,
        "bm25_artifact_chunk_topk": artifacts.bm25_topk,
        "tech_token_topk": DEFAULT_TECH_TOPK,
        "tech_tokens": tokens,
        "lanes": {"bm25": True, "tech_tokens": True, "dense": dense.on},
        "dense_model_id": dense.model_id,
        "dense_error": dense.error,
        "dense_modes": dict(dense.mode),
        "dense_candidate_rows": dict(dense.candidates),
        "hnsw_ef_search": settings.embeddings_hnsw_ef_search if dense.on else None,
    }
    if rerank is not None and rerank.on:   # keys of the rerank stage only when it is configured
        notes["reranked_from"] = rerank.scored
        notes["rerank_model_id"] = rerank.model_id
        notes["rerank_error"] = rerank.error
    if dedupe is not None and dedupe.on:   # likewise
        notes["dedupe_cosine"] = dedupe.cosine
        notes["dedupe_dropped"] = dict(dedupe.dropped)
    if lanes is not None and any("bm25_ngram" in by_name for by_name in lanes.values()):   # likewise: the lane ran
        notes["lanes"] = {"bm25": True, "bm25_ngram": True, "tech_tokens": True, "dense": dense.on}
    if _dense_per_call_cap():   # likewise
        notes["dense_per_call_cap"] = _dense_per_call_cap()
    if _dense_mmr() is not None:   # likewise
        notes["dense_mmr_lambda"] = _dense_mmr().lam
    if settings.snippet_best:   # likewise
        notes["snippet_mode"] = "best"
    return notes


def _snippet_windows(be, query: str, side: _Side, ranked) -> Optional[Dict[Any, Tuple[int, int]]]:
    """settings.snippet_best: one question to the backend per side, for the ranked rows `_pack` is about to walk."""
    ids = [row[side.id_field] for row, _, _ in ranked]
    ask = getattr(be, "snippet_windows", None)   # (a duck-typed backend may not have the method)
    found = ask(side.table, query, ids) if ask is not None and ids else None
    return None if found is None else dict(zip(ids, found))


def retrieve_evidence(payload: RetrieveRequest, backend: Optional[RetrieveBackend] = None) -> Dict[str, Any]:
    """The /retrieve entry point (S9; reference: /root/reference/app/retrieve.py:392-688): lexical lanes and
    the dense lane per table -> RRF -> either the fused id list or a budgeted evidence pack.  Built from the
    response contract (ten reference-captured scenarios), table-driven over `_SIDES`."""
    from uuid import uuid4

    from .tech_tokens import extract_tech_tokens

    be = backend if backend is not None else _backend
    if be is None:
        raise RuntimeError("retrieve_evidence: no backend registered (set_backend)")
    head: Dict[str, Any] = {"query_id": str(uuid4())}
    ids_only = payload.return_style == "ids_only"
    budget = payload.budget or Budget()
    query = payload.query.strip()
    # facet counts over the rows that pass the filters (not over the ranked hits), whatever the query text and the lanes
    # do; a request without `facets` gets no key
    facets: Dict[str, Any] = {}
    if getattr(payload, "facets", None):
        call_ids = be.resolve_call_ids(payload.filters)
        facets = {"facets": {s.table: be.facets(s.table, payload.filters, call_ids, list(payload.facets),
                                                int(payload.facet_top)) for s in _QUERY_ORDER}}
    if not query:
        if ids_only:
            return {**head, "retrieved_ids": [], **facets}
        return {**head, "intent": payload.intent, "budget": budget.model_dump(),
                **{s.out: [] for s in _SIDES}, "notes": {"error": "empty query"}, **facets}

    tokens = extract_tech_tokens(query)
    dense = _DenseState()
    dense.embed(query)
    lanes = _gather_lanes(be, query, tokens, payload.filters, dense)
    fused = {s.table: _rrf_merge(lanes[s.table], s.id_field) for s in _SIDES}
    dedupe = _DedupeState()
    fused = dedupe.apply(be, fused)
    rerank = _RerankState()
    fused = rerank.apply(query, fused)

    if ids_only:
        flat = [(-score, s.rank, row[s.id_field], s.tag) for s in _SIDES for row, _, score in fused[s.table]]
        flat.sort(key=lambda t: t[:3])
        response = {**head, "retrieved_ids": [f"{tag}:{rid}" for _, _, rid, tag in flat]}
    else:
        purse = _Purse(budget)
        packed = {}
        for s in _SIDES:  # artifacts are packed first and share the purse with the quotes
            cap = None if s.list_cap is None else min(s.list_cap, budget.max_evidence_items)
            if settings.snippet_best:   # (off: no new call, the snippets are the head clips)
                packed[s.out] = _pack(fused[s.table], s, purse, cap, _snippet_windows(be, query, s, fused[s.table]))
            else:
                packed[s.out] = _pack(fused[s.table], s, purse, cap)
        response = {**head, "intent": payload.intent, "budget": budget.model_dump(), **packed,
                    "notes": {"retrieval": _retrieval_notes(tokens, dense, rerank, dedupe, lanes)}}
    response.update(facets)
    if payload.debug:
        response["debug"] = _debug_section(lanes, dense)
        if dedupe.on:
            response["debug"]["dedupe"] = {key: list(pairs) for key, pairs in dedupe.pairs.items()}
    return response
