"""ctypes binding of libcrag_dense.so (C ABI: include/crag_dense.h).

The product path has no CPU fallback: if the HIP library is missing or fails to load, every
entry point raises NativeLibraryError loudly.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from pathlib import Path
from typing import Optional

_CSRC = Path(__file__).resolve().parent / "csrc"
# CRAG_DENSE_LIB: deployments that install the library elsewhere
LIB_PATH = Path(os.environ["CRAG_DENSE_LIB"]) if os.environ.get("CRAG_DENSE_LIB") else _CSRC / "libcrag_dense.so"

CRAG_MAX_K = 128
CRAG_DIM = 1024
CRAG_DEDUPE_MAX_WIDTH = 256
CRAG_SUBSET_MAX_WIDTH = 4096
CRAG_GROUP_MAX_PER = 8
CRAG_MMR_MAX_WIDTH = 256
CRAG_FILTER_MAX_QUERIES = 64
CRAG_ATTR_MAX_QUERIES = 64
CRAG_ATTR_MAX_CLAUSES = 8
CRAG_ATTR_MAX_KEYS = 512
CRAG_FACET_MAX_QUERIES = 64
CRAG_FACET_MAX_NAMESPACES = 16
CRAG_FACET_MAX_TOP = 64
CRAG_E2BIG = -5
CRAG_EINVAL = -1
CRAG_NGRAM_TILE = 4096
CRAG_DECODE_MAX_SEQS = 8
CRAG_DECODE_MAX_ROWS = 8
CRAG_DECODE_SPLIT = 128
CRAG_LM_HEAD_MAX_BANNED = 64
CRAG_EXTEND_BLOCK = 32
CRAG_EXTEND_TILE = 32
CRAG_EXTEND_SPLIT = 512
CRAG_EXTEND_SPLIT_ROWS = 512
CRAG_GRAMMAR_MAX_STATES = 4096
CRAG_GRAMMAR_MAX_CLASSES = 64
CRAG_GRAMMAR_DEAD = 0xFFFF
CRAG_SAMPLE_MIN_TEMPERATURE = 0.01
CRAG_SAMPLE_MAX_TEMPERATURE = 100.0

# every symbol include/crag_dense.h declares: name -> (restype, argtypes)
_c = ctypes
_P = _c.c_void_p
SIGNATURES = {
    "crag_last_error": (_c.c_char_p, []),
    "crag_version": (_c.c_char_p, []),
    "crag_device_count": (_c.c_int, []),
    "crag_index_create": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int64, _c.POINTER(_P)]),
    "crag_index_destroy": (_c.c_int, [_P]),
    "crag_index_add": (_c.c_int, [_P, _P, _P, _c.c_int64]),
    "crag_index_update": (_c.c_int, [_P, _c.c_int64, _P, _c.c_int64]),
    "crag_index_remove": (_c.c_int, [_P, _P, _c.c_int64, _c.POINTER(_c.c_int64)]),
    "crag_index_compact": (_c.c_int, [_P, _P, _c.POINTER(_c.c_int64)]),
    "crag_index_insert": (_c.c_int, [_P, _P, _P, _c.c_int64]),
    "crag_index_size": (_c.c_int64, [_P]),
    "crag_index_capacity": (_c.c_int64, [_P]),
    "crag_index_dim": (_c.c_int, [_P]),
    "crag_index_get_rows": (_c.c_int, [_P, _c.c_int64, _c.c_int64, _P, _P]),
    "crag_index_count_eligible": (_c.c_int, [_P, _P, _c.POINTER(_c.c_int64)]),
    "crag_index_search": (_c.c_int, [_P, _P, _c.c_int, _c.c_int, _P, _c.c_int64, _P, _P, _P]),
    "crag_index_search_async": (_c.c_int, [_P, _P, _c.c_int, _c.c_int, _P, _c.c_int64, _P, _P, _P, _P]),
    "crag_merge_topk": (_c.c_int, [_c.c_int, _P, _P, _P, _c.c_int, _c.c_int, _c.c_int, _P, _P, _P, _P]),
    "crag_result_record_bytes": (_c.c_int64, [_c.c_int, _c.c_int]),
    "crag_merge_topk_packed": (_c.c_int, [_c.c_int, _P, _c.c_int, _c.c_int, _c.c_int, _P, _P, _P, _P]),
    "crag_rrf_fuse": (_c.c_int, [_c.c_int, _P, _P, _P, _c.c_int, _c.c_int, _c.c_int, _P, _P, _P, _P, _P]),
    "crag_tech_lane": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _P, _P, _c.c_int, _c.c_int, _P, _c.c_int64, _P, _P, _P, _P]),
    "crag_upload_slot_create": (_P, []),
    "crag_upload_slot_destroy": (None, [_P]),
    "crag_tech_lane_host": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _P, _P, _c.c_int, _c.c_int, _P, _c.c_int64, _P, _P, _P,
                                       _P, _P]),
    "crag_bm25_scratch_bytes": (_c.c_int64, [_c.c_int64, _c.c_int, _c.c_int]),
    "crag_bm25_lane_host": (_c.c_int, [_P, _P, _P, _P, _P, _c.c_int64, _c.c_int64, _c.c_float, _P, _P, _P, _c.c_int, _c.c_int,
                                       _P, _c.c_int64, _P, _P, _c.c_int64, _P, _P, _P, _P]),
    "crag_bm25_clause_masks_host": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_int64, _P, _P, _P, _P, _c.c_int, _P,
                                               _c.c_int64, _P, _P, _c.c_int64, _P]),
    "crag_bm25_expand_scratch_bytes": (_c.c_int64, [_c.c_int64, _c.c_int]),
    "crag_bm25_expand_host": (_c.c_int, [_P, _P, _P, _c.c_int64, _P, _P, _P, _c.c_int, _P, _P, _c.c_int64, _P, _P, _P, _P,
                                         _P]),
    "crag_bm25_group_masks_host": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _P, _P, _P, _c.c_int, _P, _c.c_int64,
                                              _P, _P, _c.c_int64, _P]),
    "crag_bm25_snippets_host": (_c.c_int, [_P, _P, _P, _P, _c.c_int64, _c.c_int64, _P, _P, _P, _P, _P, _c.c_int, _c.c_int, _P,
                                           _P, _P, _P, _P, _P]),
    "crag_ngram_scratch_bytes": (_c.c_int64, [_c.c_int64, _c.c_int64]),
    "crag_ngram_extract": (_c.c_int, [_P, _c.c_int64, _P, _c.c_int64, _P, _P, _P, _P, _c.c_int64, _P]),
    "crag_ngram_heads": (_c.c_int, [_P, _P, _c.c_int64, _P, _P]),
    "crag_ngram_emit": (_c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _P, _P, _P, _P, _P, _c.c_int64, _P]),
    "crag_filter_masks_host": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _P, _P, _c.c_int, _P, _P, _c.c_int64, _P]),
    "crag_attr_masks_host": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int64, _P, _P, _c.c_int, _P, _c.c_int, _P, _c.c_int64, _P, _P,
                                        _c.c_int64, _P]),
    "crag_facet_workspace_bytes": (_c.c_int64, [_c.c_int64, _c.c_int, _c.c_int64, _c.c_int]),
    "crag_facet_counts_host": (_c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int64, _c.c_int64, _P, _c.c_int64, _P, _P, _c.c_int,
                                          _c.c_int, _c.c_int, _P, _c.c_int64, _P, _P, _P, _P, _P]),
    "crag_index_profile_enable": (_c.c_int, [_P, _c.c_int]),
    "crag_index_profile_read": (_c.c_int, [_P, _c.POINTER(_c.c_int64), _c.POINTER(_c.c_double),
                                           _c.POINTER(_c.c_double)]),
    "crag_index_profile_read_ex": (_c.c_int, [_P, _c.POINTER(_c.c_int64), _c.POINTER(_c.c_double),
                                              _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    "crag_index_last_scan_kernel": (_c.c_char_p, [_P]),
    "crag_index_scan_waits": (_c.c_char_p, [_P]),
    "crag_index_prefilter_row_bytes": (_c.c_int64, [_P]),
    "crag_index_search_pipelined": (_c.c_int, [_P, _P, _c.c_int, _c.c_int, _P, _c.c_int64, _P, _P, _P, _P, _c.c_int]),
    "crag_index_join": (_c.c_int, [_P, _P]),
    "crag_index_dedupe_async": (_c.c_int, [_P, _P, _P, _c.c_int, _c.c_int, _c.c_float, _P, _P, _P, _P, _P]),
    "crag_index_search_ids_scratch_bytes": (_c.c_int64, [_c.c_int, _c.c_int]),
    "crag_index_search_ids_async": (_c.c_int, [_P, _P, _c.c_int, _P, _P, _c.c_int, _c.c_int64, _c.c_int, _P, _P, _P, _P, _P,
                                               _c.c_int64, _P]),
    "crag_index_search_grouped_scratch_bytes": (_c.c_int64, [_c.c_int, _c.c_int64, _c.c_int]),
    "crag_index_search_grouped_async": (_c.c_int, [_P, _P, _c.c_int, _c.c_int, _P, _c.c_int64, _c.c_int, _P, _c.c_int64,
                                                   _P, _P, _P, _P, _P, _c.c_int64, _P]),
    "crag_index_mmr_scratch_bytes": (_c.c_int64, [_c.c_int, _c.c_int]),
    "crag_index_mmr_async": (_c.c_int, [_P, _P, _P, _P, _c.c_int, _c.c_int, _c.c_float, _c.c_int, _P, _P, _P, _P, _P, _P,
                                        _P, _c.c_int64, _P]),
    "crag_index_phase_trace": (_c.c_int, [_P, _c.POINTER(_c.c_uint64)]),
    "crag_index_prefilter_stats": (_c.c_int, [_P, _c.POINTER(_c.c_int64), _c.POINTER(_c.c_int64),
                                              _c.POINTER(_c.c_int64)]),
    "crag_index_scan_geometry": (_c.c_int, [_P, _c.c_int, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int),
                                            _c.POINTER(_c.c_int), _c.POINTER(_c.c_int64)]),
    # include/crag_encoder.h
    "crag_enc_embed_gather": (_c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int, _c.c_int64, _P]),
    "crag_enc_rmsnorm": (_c.c_int, [_P, _P, _P, _P, _P, _c.c_int64, _c.c_int, _c.c_float, _P]),
    "crag_enc_qk_norm_rope": (_c.c_int, [_P, _P, _P, _P, _P, _c.c_int64, _c.c_int, _c.c_int, _c.c_float, _P]),
    "crag_enc_v_transpose": (_c.c_int, [_P, _P, _P, _c.c_int64, _c.c_int, _c.c_int, _P]),
    "crag_enc_attention": (_c.c_int, [_P, _P, _P, _P, _P, _P, _P, _c.c_int, _c.c_int64, _c.c_int, _c.c_int,
                                      _c.c_float, _P]),
    "crag_enc_swiglu": (_c.c_int, [_P, _P, _c.c_int64, _c.c_int, _P]),
    "crag_enc_skinny_gemm": (_c.c_int, [_P, _P, _P, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _P]),
    "crag_enc_qk_rope_vt": (_c.c_int, [_P, _P, _P, _P, _P, _c.c_int64, _c.c_int, _c.c_int, _c.c_float, _P, _P, _c.c_int64, _P]),
    "crag_enc_pool_normalize": (_c.c_int, [_P, _P, _P, _P, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_float, _P]),
    "crag_enc_pool_normalize_add": (_c.c_int, [_P, _P, _P, _P, _P, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_float, _P]),
    "crag_enc_pool_normalize_rows": (_c.c_int, [_P, _P, _P, _P, _P, _c.c_int, _c.c_int, _c.c_int, _c.c_float, _P]),
    "crag_enc_small_gemm": (_c.c_int, [_P, _P, _P, _P, _P, _P, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                       _c.c_float, _P]),
    "crag_enc_wide_partial_bytes": (_c.c_int64, [_c.c_int, _c.c_int, _c.c_int]),
    "crag_enc_wide_gemm": (_c.c_int, [_P, _P, _P, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _P]),
    "crag_enc_wide_gemm_direct": (_c.c_int, [_P, _P, _P, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _P]),
    "crag_enc_wide_reduce": (_c.c_int, [_P, _P, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _P]),
    "crag_enc_wide_gemm_rows": (_c.c_int, [_P, _P, _P, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _P]),
    "crag_enc_rmsnorm_partials": (_c.c_int, [_P, _c.c_int, _c.c_int, _P, _P, _P, _P, _c.c_int, _c.c_int, _c.c_float, _P]),
    "crag_enc_small_attention": (_c.c_int, [_P, _P, _P, _P, _c.c_int, _P, _P, _c.c_int, _c.c_int, _c.c_int, _c.c_float,
                                            _c.c_float, _P]),
    "crag_enc_small_attention_seqs": (_c.c_int, [_P, _P, _P, _P, _c.c_int, _P, _P, _c.c_int, _c.c_int, _P, _c.c_int,
                                                 _c.c_int, _c.c_float, _c.c_float, _P]),
    "crag_enc_small_attention_seqs_parts": (_c.c_int, [_P, _c.c_int, _c.c_int, _P, _P, _P, _c.c_int, _P, _P, _c.c_int,
                                                       _c.c_int, _P, _c.c_int, _c.c_int, _c.c_float, _c.c_float, _P]),
    "crag_enc_attention_prefixed": (_c.c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _c.c_int, _c.c_int64, _c.c_int, _c.c_int,
                                               _c.c_float, _P]),
    "crag_enc_rerank_head": (_c.c_int, [_P, _P, _P, _P, _P, _P, _c.c_int, _c.c_int, _c.c_float, _P]),
    "crag_enc_decode_workspace_bytes": (_c.c_int64, [_c.c_int, _c.c_int, _c.c_int]),
    "crag_enc_decode_attention": (_c.c_int, [_P, _P, _P, _P, _c.c_int, _P, _P, _c.c_int, _c.c_int, _P, _P, _c.c_int, _c.c_int,
                                             _c.c_int, _c.c_float, _c.c_float, _P, _c.c_int64, _P, _P]),
    "crag_enc_decode_attention_shared": (_c.c_int, [_P, _P, _P, _P, _c.c_int, _P, _P, _c.c_int, _c.c_int, _P, _P, _P, _P,
                                                    _c.c_int, _c.c_int, _c.c_int, _c.c_float, _c.c_float, _P, _c.c_int64,
                                                    _P, _P]),
    "crag_enc_decode_attention_rows": (_c.c_int, [_P, _P, _P, _P, _c.c_int, _P, _P, _c.c_int, _c.c_int, _P, _P, _P, _P, _P,
                                                  _c.c_int, _c.c_int, _c.c_int, _c.c_float, _c.c_float, _P, _c.c_int64,
                                                  _P, _P]),
    "crag_enc_lm_head": (_c.c_int, [_P, _P, _P, _P, _P, _P, _P, _c.c_int, _c.c_int, _c.c_int, _c.c_int64, _c.c_float, _P]),
    "crag_enc_extend_workspace_bytes": (_c.c_int64, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "crag_enc_extend_attention": (_c.c_int, [_P, _P, _P, _P, _c.c_int, _P, _P, _c.c_int, _c.c_int, _P, _P, _P, _c.c_int,
                                             _c.c_int, _c.c_int, _c.c_float, _c.c_float, _P, _c.c_int64, _P, _P]),
    "crag_enc_grammar_argmax": (_c.c_int, [_P, _c.c_int64, _P, _P, _P, _P, _P, _P, _c.c_int, _c.c_int, _P, _P, _P, _c.c_int,
                                           _P]),
    "crag_enc_sample": (_c.c_int, [_P, _c.c_int64, _P, _P, _P, _P, _P, _P, _c.c_uint64, _c.c_uint32, _P, _P, _P, _c.c_int, _P]),
    "crag_enc_grammar_advance": (_c.c_int, [_P, _P, _P, _c.c_int64, _P, _P, _c.c_int, _c.c_int, _P, _P, _c.c_int, _P]),
    "crag_enc_logprobs": (_c.c_int, [_P, _c.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _c.c_int, _c.c_int, _P]),
    "crag_enc_adjust_workspace_bytes": (_c.c_int64, [_c.c_int, _c.c_int64]),
    "crag_enc_adjust_logits": (_c.c_int, [_P, _P, _c.c_int64, _P, _c.c_int64, _c.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                          _P, _P, _P, _P, _c.c_int64, _c.c_int, _P]),
}


class NativeLibraryError(RuntimeError):
    """libcrag_dense.so is missing, failed to load, or a call into it failed."""


_lib: Optional[ctypes.CDLL] = None


def build_native(force: bool = False) -> Path:
    """Compile libcrag_dense.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", str(_CSRC)] + (["-B"] if force else [])
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise NativeLibraryError(f"building libcrag_dense.so failed:\n{proc.stdout}\n{proc.stderr}")
    return LIB_PATH


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise NativeLibraryError(
            f"{LIB_PATH} not found: the dense lane has no CPU fallback. Build it with "
            f"`python -c 'import __graft_entry__ as g; g.build()'` or `make -C {_CSRC}`.")
    try:
        lib = ctypes.CDLL(str(LIB_PATH))
    except OSError as exc:
        raise NativeLibraryError(f"failed to load {LIB_PATH}: {exc}") from exc
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            raise NativeLibraryError(f"{LIB_PATH} does not export {name}") from exc
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def last_error() -> str:
    msg = load().crag_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise NativeLibraryError(f"{what} failed (code {rc}): {last_error()}")


class UploadRing:
    """Per stream a ring of four upload slots, for the lanes that take host query data (the *_host entry points): a
    crag_upload_slot of the library is a pinned host buffer, its device twin and the event of its last upload, so a
    call may fill a slot while the three calls before it on the stream are still in flight.  Slots are created on
    first use and freed by `close` (also when the ring is collected)."""
    SIZE = 4

    def __init__(self, device) -> None:
        self.device = device
        self._rings: dict = {}      # stream -> [calls so far, handles]

    def take(self, stream: int):
        """The stream's next slot: (its place in the ring, its handle) -- the place for owners that keep something of
        their own per slot."""
        ring = self._rings.setdefault(stream, [0, []])
        if len(ring[1]) < self.SIZE:
            import torch
            with torch.cuda.device(self.device):
                handle = load().crag_upload_slot_create()
            if not handle:
                raise NativeLibraryError(f"crag_upload_slot_create failed: {last_error()}")
            ring[1].append(handle)
        at = ring[0] % len(ring[1])
        ring[0] += 1
        return at, ring[1][at]

    def slot(self, stream: int):
        return self.take(stream)[1]

    def close(self) -> None:
        rings, self._rings = getattr(self, "_rings", {}), {}
        for _, handles in rings.values():
            for handle in handles:
                load().crag_upload_slot_destroy(handle)

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown: the library may be gone already
            pass
