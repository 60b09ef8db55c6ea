"""Filter row masks built on the GPU -- the device counterpart of DenseTable.filter_mask, i.e. of the reference's
_build_filter_clause (app/retrieve.py:93-120), for up to 64 queries per launch (crag_filter_masks_host).

The filter columns of a table live in HBM beside its vectors (FilterColumns: call_started_at in microseconds and the
dense number of the row's call, 12 bytes per row); a request's predicates are compiled on the host into two date bounds
per query and, transposed, one 64-bit query set per CALL (compile_predicates: its cost is in the number of calls and
listed ids, never in the number of rows); the kernel evaluates them for every row and writes the packed masks the lanes
take.  DenseTable.filter_mask stays the public host form of the same predicate.

Row-level predicates -- entity, speaker and kind -- go the same way through a second kernel
(crag_attr_masks_host): a row's attributes are (namespace, value) pairs, namespace one of "speaker", "kind",
"entity:" + LABEL; a table's AttributeColumns hold them as a CSR of dictionary ids in HBM (8 bytes per row + 4 per
attribute); compile_attr_predicates turns a request's entity_filters / speakers / kinds into clauses of keys (a cost in
keys, never in rows), and a row passes iff every clause is hit by one of its attributes.  A namespace a table lacks is
NULL there and fails every clause over it, so a `speakers` filter returns no artifact rows.

Facet counts -- which speakers, kinds and entities the rows under a filter carry, and how many rows hold
each -- come from a third set of columns, FacetColumns: the same attributes renumbered by (namespace, value) and stored as
postings (8 bytes per posting + 8 per attribute of HBM), counted by crag_facet_counts_host under the masks the two
kernels above write.  facets_host is the host form of the rule."""
from __future__ import annotations

import ctypes
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _native

MAX_QUERIES = _native.CRAG_FILTER_MAX_QUERIES
MAX_CLAUSES = _native.CRAG_ATTR_MAX_CLAUSES
MAX_KEYS = _native.CRAG_ATTR_MAX_KEYS
NO_LOWER = np.iinfo(np.int64).min   # date_from of a query without a lower bound; also a row's NULL / NaT timestamp
NO_UPPER = np.iinfo(np.int64).max   # date_to of a query without an upper bound


def mask_bytes(n_rows: int) -> int:
    """Bytes of one packed mask over n_rows rows (the minimal mask_stride)."""
    return ((int(n_rows) + 31) // 32) * 4


def _nonempty(a: np.ndarray) -> np.ndarray:
    """`a`, or one zero of its dtype when `a` is empty: an upload or a pointer argument always has a valid address."""
    return a if a.size else np.zeros(1, dtype=a.dtype)


def _halve_on_e2big(call, q0: int, nq: int, too_big) -> None:
    """Queries [q0, q0 + nq) through `call(q0, nq)`, which returns the entry's code after raising for every error but
    CRAG_E2BIG: a batch that is too big for one call goes as its two halves, in order; a single query that is too big
    raises `too_big(q0)`, the caller's ValueError."""
    if call(q0, nq) != _native.CRAG_E2BIG:
        return
    if nq == 1:
        raise too_big(q0)
    half = nq // 2
    _halve_on_e2big(call, q0, half, too_big)
    _halve_on_e2big(call, q0 + half, nq - half, too_big)


class _RingColumns:
    """Device columns whose kernel takes host arguments: they go through one upload slot per stream of `_ring`."""

    def _slot(self, stream: int):
        return self._ring.slot(stream)

    def close(self) -> None:
        self._ring.close()


def _mask_frame(cols, noun: str, nq: int, stride: Optional[int], out, stream: Optional[int]):
    """What the two `masks` methods do before their kernel: the device check, the bounds of nq, the default stride
    (minimal) and stream (torch's current one), `out` allocated on that stream or validated.  Returns (out, stride,
    stream); stride == 0 is an empty table, whose runs are empty: the caller returns `out` as it is."""
    import torch
    if cols.device is None:
        raise _native.NativeLibraryError(f"these {type(cols).__name__} were built without a device")
    if not 1 <= nq <= MAX_QUERIES:
        raise ValueError(f"{noun} batch holds 1 to {MAX_QUERIES} queries")
    stride = mask_bytes(cols.n) if stride is None else int(stride)
    if stream is None:
        stream = torch.cuda.current_stream(cols.device).cuda_stream
    if out is None:
        from .fusion import _on_stream
        with _on_stream(stream, cols.device):
            out = torch.empty((nq, stride), dtype=torch.uint8, device=cols.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (nq, stride) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 [{nq}, {stride}] tensor")
    return out, stride, stream


class FilterColumns(_RingColumns):
    """The filter columns of one DenseTable: per row `started_us` (int64 microseconds since the epoch, NO_LOWER for
    NaT) and `call_slot` (int32: the dense number of the row's call in `slot_of`, numbered by first appearance), built in
    ONE host pass over the rows -- per table generation, not per request.  With a `device` the two arrays are uploaded
    (d_started_us, d_call_slot: 12 bytes per row of HBM); without one the object is plain arrays, which is all
    compile_predicates needs."""

    def __init__(self, call_started_at, call_ids, device=None, generation: Optional[int] = None) -> None:
        self.started_us = np.ascontiguousarray(np.asarray(call_started_at, dtype="datetime64[us]").astype(np.int64))
        self.n = int(self.started_us.size)
        if len(call_ids) != self.n:
            raise ValueError("call_started_at and call_ids must have one entry per row")
        slot_of: Dict[Any, int] = {}
        number = slot_of.setdefault
        self.call_slot = np.fromiter((number(c, len(slot_of)) for c in call_ids), dtype=np.int32, count=self.n)
        self.slot_of = slot_of
        self.n_calls = len(slot_of)
        self.generation = generation
        self.device = device
        self.d_started_us = self.d_call_slot = None
        self._ring = _native.UploadRing(device)
        if device is not None:
            import torch
            self.d_started_us = torch.from_numpy(self.started_us).to(device)
            self.d_call_slot = torch.from_numpy(self.call_slot).to(device)

    def _slot(self, stream: int):
        return self._ring.slot(stream)

    def close(self) -> None:
        self._ring.close()

    def masks(self, qset: Optional[np.ndarray], date_from: np.ndarray, date_to: np.ndarray, stride: Optional[int] = None,
              out=None, stream: Optional[int] = None):
        """Enqueue the kernel for compiled predicates on `stream` (default: torch's current stream): a uint8 CUDA
        tensor [nq, stride] (stride: a multiple of 4 >= mask_bytes(n), default minimal), every byte written.  `out`: a
        tensor of that shape to write into (it may hold anything).  No host synchronisation."""
        nq = int(date_from.size)
        if int(date_to.size) != nq:
            raise ValueError("date_from and date_to hold one bound per query each")
        out, stride, stream = _mask_frame(self, "a filter", nq, stride, out, stream)
        if stride == 0:   # an empty table: the runs are empty
            return out
        date_from = np.ascontiguousarray(date_from, dtype=np.int64)
        date_to = np.ascontiguousarray(date_to, dtype=np.int64)
        qptr = None
        if qset is not None:
            qset = np.ascontiguousarray(qset, dtype=np.uint64)
            if qset.size != self.n_calls:
                raise ValueError("qset must have one word per call")
            qset = _nonempty(qset)   # (scoped, no calls)
            qptr = qset.ctypes.data
        rc = _native.load().crag_filter_masks_host(
            self.d_started_us.data_ptr() if self.n else None, self.d_call_slot.data_ptr() if self.n else None, self.n,
            self.n_calls, qptr, date_from.ctypes.data, date_to.ctypes.data, nq, self._slot(stream), out.data_ptr(), stride,
            ctypes.c_void_p(stream))
        _native.check(rc, "crag_filter_masks_host")
        return out


def _us(dt) -> int:
    from .retrieve import _naive_utc
    return int(np.datetime64(_naive_utc(dt), "us").astype(np.int64))


def compile_predicates(columns: FilterColumns, call_tags: Dict[Any, Sequence[str]],
                       batch: Sequence[Tuple[Any, Optional[Sequence[Any]]]]
                       ) -> Tuple[Optional[np.ndarray], np.ndarray, np.ndarray]:
    """batch: up to 64 (filters, call_ids) pairs, the arguments of DenseTable.filter_mask.  Returns (qset, date_from,
    date_to): uint64 [n_calls] or None when no query is call-scoped, int64 [nq] microseconds with NO_LOWER / NO_UPPER
    for an open side.  Semantics are filter_mask's, quirks included: nothing applies unless `filters` is truthy
    (call_ids too); call_ids == [] admits nothing; tags mean an overlap with call_tags[call], a call absent from
    call_tags has none; call ids and tags intersect; bounds go through _naive_utc."""
    nq = len(batch)
    if nq > MAX_QUERIES:
        raise ValueError(f"a filter batch holds at most {MAX_QUERIES} queries (got {nq}): the caller splits it")
    date_from = np.full(nq, NO_LOWER, dtype=np.int64)
    date_to = np.full(nq, NO_UPPER, dtype=np.int64)
    slot_of = columns.slot_of
    scoped: Dict[int, Sequence[int]] = {}
    for q, (filters, call_ids) in enumerate(batch):
        if not filters:
            continue
        if filters.date_from:
            date_from[q] = _us(filters.date_from)
        if filters.date_to:
            date_to[q] = _us(filters.date_to)
        admitted = None
        if call_ids is not None:
            admitted = {slot_of[c] for c in set(call_ids) if c in slot_of}
        if filters.call_tags:
            tags = set(filters.call_tags)
            tagged = {slot_of[c] for c, t in call_tags.items() if c in slot_of and tags.intersection(t or ())}
            admitted = tagged if admitted is None else (admitted & tagged)
        if admitted is not None:
            scoped[q] = sorted(admitted)
    if not scoped:
        return None, date_from, date_to
    open_bits = 0
    for q in range(nq):
        if q not in scoped:
            open_bits |= 1 << q
    qset = np.full(columns.n_calls, open_bits, dtype=np.uint64)
    for q, slots in scoped.items():
        if slots:
            qset[np.asarray(slots, dtype=np.int64)] |= np.uint64(1 << q)
    return qset, date_from, date_to


def is_unfiltered(qset: Optional[np.ndarray], date_from: np.ndarray, date_to: np.ndarray) -> bool:
    """No query of the compiled batch restricts anything (for one query: DenseTable.filter_mask returns None)."""
    return qset is None and bool(np.all(date_from == NO_LOWER)) and bool(np.all(date_to == NO_UPPER))


# ---- row-level predicates: entity, speaker, kind (crag_attr_masks_host) -----------------------------
Attr = Tuple[str, str]   # (namespace, normalised value)


def normalize_attr(value) -> Optional[str]:
    """The one normal form of an attribute value, used on the row side and the query side: whitespace runs collapsed
    to one space, ends stripped, casefolded.  None or an empty value is no attribute: None."""
    if value is None:
        return None
    return " ".join(str(value).split()).casefold() or None


def entity_namespace(label) -> str:
    return "entity:" + str(label if label is not None else "").strip().upper()


def _entity_pair(entity) -> Tuple[Any, Any]:
    if isinstance(entity, dict):
        return entity.get("label"), entity.get("value")
    label, value = entity
    return label, value


def row_attributes(n: int, speakers: Optional[Sequence[Any]], kinds: Optional[Sequence[Any]],
                   entities: Optional[Sequence[Iterable[Any]]]) -> List[List[Attr]]:
    """The attributes of n rows from their `speaker` entries, `kind` entries and entity lists ((label, value) pairs or
    {"label", "value"} dicts); an argument that is None is a namespace the table lacks."""
    rows: List[List[Attr]] = [[] for _ in range(n)]
    for namespace, column in (("speaker", speakers), ("kind", kinds)):
        if column is None:
            continue
        if len(column) != n:
            raise ValueError(f"the {namespace} column must have one entry per row")
        for attrs, raw in zip(rows, column):
            value = normalize_attr(raw)
            if value is not None:
                attrs.append((namespace, value))
    if entities is not None:
        if len(entities) != n:
            raise ValueError("entities must have one entry per row")
        for attrs, listed in zip(rows, entities):
            for entity in listed or ():
                label, raw = _entity_pair(entity)
                value = normalize_attr(raw)
                if value is not None:
                    attrs.append((entity_namespace(label), value))
    return rows


def attr_clauses(filters) -> List[List[Attr]]:
    """The clauses of one request: each entity_filters entry is a clause of one key, `speakers` is one clause of all its
    keys, `kinds` likewise; a falsy field is not applied (as call_tags).  A value that normalises to nothing is no key,
    so its clause may be left without any and then admits nothing.  More than 8 clauses: ValueError."""
    clauses: List[List[Attr]] = []
    if not filters:
        return clauses
    for entity in getattr(filters, "entity_filters", None) or ():
        label, raw = _entity_pair(entity)
        value = normalize_attr(raw)
        clauses.append([] if value is None else [(entity_namespace(label), value)])
    for namespace, field in (("speaker", "speakers"), ("kind", "kinds")):
        listed = getattr(filters, field, None)
        if listed:
            values = [normalize_attr(v) for v in listed]
            clauses.append([(namespace, v) for v in values if v is not None])
    if len(clauses) > MAX_CLAUSES:
        raise ValueError(f"a request holds at most {MAX_CLAUSES} attribute clauses (got {len(clauses)})")
    return clauses


class AttributeColumns(_RingColumns):
    """The attribute columns of one DenseTable: a dictionary `id_of` from (namespace, value) to an int32 id, numbered by
    first appearance (exact strings, no hashing: the BM25 vocabulary's idiom), and the rows' ids as a CSR by row position
    (`attr_ptr` int64 [n + 1], `attr_ids` int32; duplicates inside a row are kept), built in ONE host pass per table
    generation.  `row_attrs`: per row an iterable of (namespace, value) pairs already in normal form (row_attributes).
    With a `device` the two arrays are uploaded (8 bytes per row + 4 per attribute of HBM); without one the object is
    plain arrays, which is all compile_attr_predicates needs."""

    def __init__(self, row_attrs: Sequence[Iterable[Attr]], device=None, generation: Optional[int] = None) -> None:
        id_of: Dict[Attr, int] = {}
        number = id_of.setdefault
        self.n = len(row_attrs)
        ptr = np.zeros(self.n + 1, dtype=np.int64)
        ids: List[int] = []
        for i, attrs in enumerate(row_attrs):
            ids.extend(number(a, len(id_of)) for a in attrs)
            ptr[i + 1] = len(ids)
        self.attr_ptr = ptr
        self.attr_ids = np.asarray(ids, dtype=np.int32)
        self.id_of = id_of
        self.n_attrs = len(id_of)
        self.generation = generation
        self.device = device
        self.d_attr_ptr = self.d_attr_ids = None
        self._ring = _native.UploadRing(device)
        if device is not None:
            import torch
            self.d_attr_ptr = torch.from_numpy(self.attr_ptr).to(device)
            self.d_attr_ids = torch.from_numpy(_nonempty(self.attr_ids)).to(device)   # (a row list without attributes)

    def masks(self, compiled: Tuple[np.ndarray, np.ndarray, np.ndarray], in_mask=None, in_stride: int = 0,
              stride: Optional[int] = None, out=None, stream: Optional[int] = None, nq: Optional[int] = None):
        """Enqueue the kernel for compiled clauses (compile_attr_predicates) on `stream` (default: torch's current
        stream): a uint8 CUDA tensor [nq, stride], every byte written.  `in_mask`: a uint8 CUDA tensor ANDed in -- one
        run shared by all queries (in_stride 0) or one run of in_stride bytes per query; it may be `out` itself with
        in_stride == stride (in place).  A batch that lists more than 512 distinct keys (CRAG_E2BIG) is split by queries
        into row slices of `out`; a single query above 512 keys is a ValueError.  `nq`: the number of queries, by default
        the rows of `out`, else the number up to the last query that has a clause.  No host synchronisation."""
        keys, key_sets, clause_sets = compiled
        clause_sets = np.ascontiguousarray(clause_sets, dtype=np.uint64)
        if nq is None:
            nq = max(int(w).bit_length() for w in clause_sets) if out is None else int(out.shape[0])
        out, stride, stream = _mask_frame(self, "an attribute", int(nq), stride, out, stream)
        if stride == 0:   # an empty table: the runs are empty
            return out
        keys = np.ascontiguousarray(keys, dtype=np.int32)
        key_sets = np.ascontiguousarray(key_sets, dtype=np.uint64).reshape(-1, MAX_CLAUSES)
        in_ptr, in_stride = None if in_mask is None else in_mask.data_ptr(), int(in_stride)
        out_ptr = out.data_ptr()

        def listed(q0: int, n: int):
            """The keys that queries [q0, q0 + n) list, and their sets as bits 0 .. n - 1."""
            sets = (key_sets >> np.uint64(q0)) & np.uint64((1 << n) - 1)
            some = sets.any(axis=1)
            return np.ascontiguousarray(keys[some]), np.ascontiguousarray(sets[some])

        def run(q0: int, n: int) -> int:
            """Queries [q0, q0 + n) of the compiled batch into their rows of the output."""
            k, s = listed(q0, n)
            c = np.ascontiguousarray((clause_sets >> np.uint64(q0)) & np.uint64((1 << n) - 1))
            rc = _native.load().crag_attr_masks_host(
                self.d_attr_ptr.data_ptr() if self.n else None, self.d_attr_ids.data_ptr() if self.n else None, self.n,
                self.n_attrs, k.ctypes.data if k.size else None, s.ctypes.data if k.size else None, int(k.size), c.ctypes.data,
                n, None if in_ptr is None else in_ptr + q0 * in_stride, in_stride, self._slot(stream), out_ptr + q0 * stride,
                stride, ctypes.c_void_p(stream))
            if rc != _native.CRAG_E2BIG:
                _native.check(rc, "crag_attr_masks_host")
            return rc

        _halve_on_e2big(run, 0, int(nq), lambda q: ValueError(
            f"one query lists {int(listed(q, 1)[0].size)} distinct attribute keys, a call takes {MAX_KEYS}"))
        return out


def compile_attr_predicates(columns: AttributeColumns, batch: Sequence[Tuple[Any, Optional[Sequence[Any]]]]
                            ) -> Optional[Tuple[np.ndarray, np.ndarray, np.ndarray]]:
    """batch: up to 64 (filters, call_ids) pairs, the arguments of DenseTable.filter_mask (the call ids play no part).
    None when no query has an attribute clause, else (keys, key_sets, clause_sets), the host arguments of
    crag_attr_masks_host: int32 [n_keys] strictly ascending dictionary ids, uint64 [n_keys, 8] with bit q of word (j, c)
    set iff clause c of query q lists key j, uint64 [8] with bit q of word c set iff query q has a clause c.  A key the
    dictionary does not hold is dropped from its clause; a clause left without keys admits nothing.  The cost is in the
    number of keys, never rows; no GPU is needed."""
    nq = len(batch)
    if nq > MAX_QUERIES:
        raise ValueError(f"a filter batch holds at most {MAX_QUERIES} queries (got {nq}): the caller splits it")
    clause_sets = np.zeros(MAX_CLAUSES, dtype=np.uint64)
    sets: Dict[int, List[int]] = {}
    id_of = columns.id_of
    for q, (filters, _call_ids) in enumerate(batch):
        for c, clause in enumerate(attr_clauses(filters)):
            clause_sets[c] |= np.uint64(1 << q)
            for key in clause:
                j = id_of.get(key)
                if j is not None:
                    sets.setdefault(j, [0] * MAX_CLAUSES)[c] |= 1 << q
    if not clause_sets.any():
        return None
    keys = np.asarray(sorted(sets), dtype=np.int32)
    key_sets = np.asarray([sets[int(j)] for j in keys], dtype=np.uint64).reshape(-1, MAX_CLAUSES)
    return keys, key_sets, clause_sets


# ---- facet counts: attribute histograms under a filter (crag_facet_counts_host) ---------------------
MAX_FACET_NAMESPACES = _native.CRAG_FACET_MAX_NAMESPACES
MAX_FACET_TOP = _native.CRAG_FACET_MAX_TOP
FACET_TABLE_BYTES = 256 << 20   # the count table a call allocates by default, at most: a larger batch is split by queries


def facet_namespace(name) -> str:
    """A requested namespace in the form row_attributes produces: "speaker", "kind", or "entity:" + LABEL with the label
    normalised by entity_namespace."""
    name = str(name).strip()
    return entity_namespace(name[len("entity:"):]) if name[:len("entity:")].lower() == "entity:" else name


def facets_host(row_attrs: Sequence[Iterable[Attr]], mask_bits, namespaces: Sequence[str], top: int
                ) -> Tuple[int, Dict[str, Tuple[List[Tuple[str, int]], int]]]:
    """The host rule of the facet counts, kept as public oracle the way DenseTable.filter_mask is for the masks.
    row_attrs: per row its (namespace, value) pairs in normal form; mask_bits: per row a truth value, or None for every
    row.  Returns (rows, {namespace as given: ([(value, count), ...], distinct)}): rows = the rows that pass; count = the
    passing rows that hold the attribute at least once; the list holds the `top` attributes of the namespace with
    count > 0 by count descending, then value ascending (str order); distinct = how many there are before the cut."""
    if not 1 <= int(top) <= MAX_FACET_TOP:
        raise ValueError(f"top must be in 1..{MAX_FACET_TOP}")
    wanted = {facet_namespace(ns) for ns in namespaces}
    tallies: Dict[str, Dict[str, int]] = {ns: {} for ns in wanted}
    rows = 0
    for i, attrs in enumerate(row_attrs):
        if mask_bits is not None and not mask_bits[i]:
            continue
        rows += 1
        for namespace, value in set(attrs):
            if namespace in wanted:
                tally = tallies[namespace]
                tally[value] = tally.get(value, 0) + 1
    out = {}
    for ns in namespaces:
        tally = tallies[facet_namespace(ns)]
        out[ns] = (sorted(tally.items(), key=lambda kv: (-kv[1], kv[0]))[:int(top)], len(tally))
    return rows, out


class FacetColumns:
    """The facet columns of one table, built from its AttributeColumns in ONE host pass of numpy sorts per table
    generation (no loop over rows):

    * facet ids: the dictionary's attributes renumbered by (namespace, value) ascending (Python str order), so that a
      namespace is one contiguous range `ranges[namespace] = (lo, hi)` and ascending facet id is ascending value -- the
      tie order of the lists, independent of the dictionary's first-appearance numbering.  `facet_keys[fid]` is the
      (namespace, value) of a facet id.
    * postings: the transpose of the CSR -- `post_ptr` int64 [n_attrs + 1], `post_rows` int32 ascending within an
      attribute, `post_fid` int32 parallel to it (a lane knows its attribute without a search); each (attribute, row)
      pair once: the duplicates a row may list are removed here.

    HBM with a `device`: 8 bytes per posting (row + facet id) + 8 per attribute.  Without one the object is plain arrays."""

    def __init__(self, attrs: AttributeColumns, device=None, generation: Optional[int] = None) -> None:
        self.n = int(attrs.n)
        self.n_attrs = int(attrs.n_attrs)
        keys = list(attrs.id_of)   # in dictionary order: keys[j] has id j
        order = sorted(range(self.n_attrs), key=keys.__getitem__)
        self.facet_keys: List[Attr] = [keys[j] for j in order]
        fid_of = np.empty(self.n_attrs, dtype=np.int64)
        fid_of[np.asarray(order, dtype=np.int64)] = np.arange(self.n_attrs, dtype=np.int64)
        self.ranges: Dict[str, Tuple[int, int]] = {}
        for fid, (namespace, _value) in enumerate(self.facet_keys):
            lo, _hi = self.ranges.get(namespace, (fid, fid))
            self.ranges[namespace] = (lo, fid + 1)
        row_of = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(attrs.attr_ptr))
        pairs = np.unique(fid_of[attrs.attr_ids] * max(self.n, 1) + row_of)   # sorted by (facet id, row), each pair once
        self.post_fid = (pairs // max(self.n, 1)).astype(np.int32)
        self.post_rows = (pairs % max(self.n, 1)).astype(np.int32)
        self.n_postings = int(pairs.size)
        self.post_ptr = np.zeros(self.n_attrs + 1, dtype=np.int64)
        np.cumsum(np.bincount(self.post_fid, minlength=self.n_attrs), out=self.post_ptr[1:])
        self.generation = generation
        self.device = device
        self.d_post_ptr = self.d_post_rows = self.d_post_fid = None
        if device is not None:
            import torch
            self.d_post_ptr = torch.from_numpy(self.post_ptr).to(device)
            self.d_post_rows = torch.from_numpy(_nonempty(self.post_rows)).to(device)
            self.d_post_fid = torch.from_numpy(_nonempty(self.post_fid)).to(device)

    def requested(self, namespaces: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
        """The ranges of the requested namespaces, (lo, hi) int32 arrays; a namespace the table lacks is (0, 0)."""
        names = [facet_namespace(ns) for ns in namespaces]
        if len(names) > MAX_FACET_NAMESPACES:
            raise ValueError(f"a facet call takes at most {MAX_FACET_NAMESPACES} namespaces (got {len(names)})")
        if len(set(names)) != len(names):
            raise ValueError("a facet call lists each namespace once")
        pairs = [self.ranges.get(ns, (0, 0)) for ns in names]
        return (np.asarray([p[0] for p in pairs], dtype=np.int32), np.asarray([p[1] for p in pairs], dtype=np.int32))

    def counts(self, namespaces: Sequence[str], masks=None, nq: Optional[int] = None, top: int = 10,
               stream: Optional[int] = None, workspace=None):
        """Enqueue the facet kernels on `stream` (default: torch's current stream).  `masks`: a uint8 CUDA tensor
        [nq, stride] in the layout filter_masks_device writes, or None for every row (then `nq`, default 1, is the number
        of queries).  Returns CUDA tensors (ids int32 [nq, R, top] with -1 beyond a list, counts int32 [nq, R, top] with 0
        beyond it -- the kernel's uint32, always below 2^31 --, distinct int32 [nq, R], rows int64 [nq]), every element
        written; R = len(namespaces).  `workspace`: a uint8 CUDA tensor to use as scratch (default: allocated for the
        call, its count table capped at FACET_TABLE_BYTES); a batch whose count table does not fit it (CRAG_E2BIG) is
        split by queries, a single query that does not fit is a ValueError.  No host synchronisation."""
        import torch
        if self.device is None:
            raise _native.NativeLibraryError("these FacetColumns were built without a device")
        lo, hi = self.requested(namespaces)
        top = int(top)
        if not 1 <= top <= MAX_FACET_TOP:
            raise ValueError(f"top must be in 1..{MAX_FACET_TOP}")
        stride = 0
        if masks is not None:
            if masks.dtype != torch.uint8 or masks.dim() != 2 or not masks.is_contiguous():
                raise ValueError("masks must be a contiguous uint8 [nq, stride] tensor")
            if nq is not None and int(nq) != int(masks.shape[0]):
                raise ValueError("nq must be the number of mask runs")
            nq, stride = int(masks.shape[0]), int(masks.shape[1])
        nq = 1 if nq is None else int(nq)
        if not 1 <= nq <= MAX_QUERIES:
            raise ValueError(f"a facet batch holds 1 to {MAX_QUERIES} queries")
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        n_ranges, width = int(lo.size), int((hi - lo).sum())
        lib = _native.load()
        from .fusion import _on_stream
        with _on_stream(stream, self.device):
            ids = torch.empty((nq, n_ranges, top), dtype=torch.int32, device=self.device)
            counts = torch.empty((nq, n_ranges, top), dtype=torch.int32, device=self.device)
            distinct = torch.empty((nq, n_ranges), dtype=torch.int32, device=self.device)
            rows = torch.empty((nq,), dtype=torch.int64, device=self.device)
            if workspace is None:
                sets = int(lib.crag_facet_workspace_bytes(self.n, 0, 0, 1 if stride else 0))
                table = int(lib.crag_facet_workspace_bytes(0, nq, width, 0))
                workspace = torch.empty((sets + max(min(table, FACET_TABLE_BYTES), 4 * width),), dtype=torch.uint8,
                                        device=self.device)
        if workspace.dtype != torch.uint8 or not workspace.is_contiguous():
            raise ValueError("workspace must be a contiguous uint8 tensor")

        def run(q0: int, n: int) -> int:
            rc = lib.crag_facet_counts_host(
                self.d_post_ptr.data_ptr(), self.d_post_rows.data_ptr(), self.d_post_fid.data_ptr(), self.n_postings,
                self.n, self.n_attrs, masks.data_ptr() + q0 * stride if stride else None, stride,
                lo.ctypes.data if n_ranges else None, hi.ctypes.data if n_ranges else None, n_ranges, n, top,
                workspace.data_ptr() if workspace.numel() else None, int(workspace.numel()),
                ids.data_ptr() + q0 * n_ranges * top * 4 if n_ranges else None,
                counts.data_ptr() + q0 * n_ranges * top * 4 if n_ranges else None,
                distinct.data_ptr() + q0 * n_ranges * 4 if n_ranges else None, rows.data_ptr() + q0 * 8,
                ctypes.c_void_p(stream))
            if rc != _native.CRAG_E2BIG:
                _native.check(rc, "crag_facet_counts_host")
            return rc

        def too_big(_q0: int) -> ValueError:
            widths = {ns: int(h - l) for ns, l, h in zip(namespaces, lo, hi)}
            return ValueError(f"one query's count table ({4 * width} bytes + the query sets) does not fit a workspace "
                              f"of {int(workspace.numel())} bytes; namespace widths: {widths}")

        _halve_on_e2big(run, 0, nq, too_big)
        return ids, counts, distinct, rows

    def lists(self, namespaces: Sequence[str], ids, counts, distinct, rows) -> List[Dict[str, Any]]:
        """The host tensors / arrays of `counts` as per query {"rows", "facets": {namespace as given: {"values":
        [{"value", "count"}], "distinct"}}}."""
        ids, counts, distinct, rows = (np.asarray(a) for a in (ids, counts, distinct, rows))
        out = []
        for q in range(rows.shape[0]):
            facets = {}
            for r, ns in enumerate(namespaces):
                values = [{"value": self.facet_keys[int(f)][1], "count": int(c)} for f, c in zip(ids[q, r], counts[q, r])
                          if f >= 0]
                facets[ns] = {"values": values, "distinct": int(distinct[q, r])}
            out.append({"rows": int(rows[q]), "facets": facets})
        return out
