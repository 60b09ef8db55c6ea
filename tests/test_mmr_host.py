"""MMR, host side (no GPU): the fp32 rule of cadence_rag_amd.mmr.mmr_host against the fp64 oracle of mmr_oracle.py on lists
whose decision gaps are large by construction, a case by hand, lambda = 1 as the plain sort; the binding and the header
agree; the scratch is sized sensibly; every bad argument is refused with a code and a message before a device is touched;
the DENSE_MMR_LAMBDA / DENSE_MMR_FETCH knobs are read, default to off, and an unset knob leaves the notes as they were."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from cadence_rag_amd import _native
from cadence_rag_amd import retrieve as rt
from cadence_rag_amd.config import Settings, settings
from cadence_rag_amd.mmr import MmrParams, mmr_host
from mmr_oracle import crafted, mmr_oracle, pair_cosines

HEADER = Path(__file__).resolve().parent.parent / "include" / "crag_dense.h"
CRAFTED = ((0.5, 12, 1), (0.7, 40, 0), (0.3, 20, 11))   # lambda, k, seed: the first seeds whose every gap is >= 1e-3


@pytest.mark.parametrize("lam,k,seed", CRAFTED)
def test_host_rule_equals_the_oracle_on_crafted_lists(lam, k, seed):
    rows, ids, rel = crafted(seed)
    cos = pair_cosines(ids, rows, ids)
    slots, values, gaps = mmr_oracle(rel, cos, lam, k, ids)
    assert slots.size == k and gaps.min() >= 1e-3            # an assertion on the construction
    plain, _, _ = mmr_oracle(rel, cos, 1.0, k, ids)
    assert not np.array_equal(slots, plain)                  # the penalty does change the order
    got, got_values = mmr_host(rel, cos.astype(np.float32), lam, k, ids)
    assert np.array_equal(got, slots)
    assert np.max(np.abs(got_values.astype(np.float64) - values)) <= 1e-6
    by_row = mmr_host(rel, lambda p, t: cos[p].astype(np.float32), lam, k, ids)   # the callable form
    assert np.array_equal(by_row[0], got) and np.array_equal(by_row[1].view(np.uint32), got_values.view(np.uint32))


def test_a_case_by_hand():
    """a, a' near-duplicates with the top relevance, b different and less relevant."""
    rel = np.asarray([0.95, 0.8, 0.6], dtype=np.float32)
    cos = np.asarray([[1.0, 0.98, 0.1], [0.98, 1.0, 0.1], [0.1, 0.1, 1.0]], dtype=np.float32)
    ids = [4, 5, 6]
    assert mmr_host(rel, cos, 1.0, 3, ids)[0].tolist() == [0, 1, 2]
    slots, values = mmr_host(rel, cos, 0.5, 3, ids)
    # step 2: b = 0.5 * 0.6 - 0.5 * 0.1 = 0.25 against a' = 0.5 * 0.8 - 0.5 * 0.98 = -0.09
    assert slots.tolist() == [0, 2, 1]
    assert np.allclose(values, [0.475, 0.25, -0.09], atol=1e-6)
    for lam, want in ((1.0, [0, 1, 2]), (0.5, [0, 2, 1])):
        got, _, gaps = mmr_oracle(rel, cos, lam, 3, ids)
        assert got.tolist() == want and gaps.min() >= 0.05
    # the first comparison SETS the penalty (it may be negative), later ones raise it; NaN pairs never count
    cos2 = np.asarray([[1.0, -0.5, np.nan], [-0.5, 1.0, np.nan], [np.nan, np.nan, np.nan]], dtype=np.float32)
    slots, values = mmr_host([0.9, 0.1, 0.3], cos2, 0.5, 3, ids)
    assert slots.tolist() == [0, 1, 2] and np.allclose(values, [0.45, 0.05 + 0.25, 0.15], atol=1e-6)
    # ignored slots: the -1 pad, a non-finite rel, a repeated id; equal values go to the lower id; k beyond the candidates
    slots, values = mmr_host([0.5, np.nan, 0.5, 0.7, 0.9, np.inf], np.full((6, 6), np.nan, dtype=np.float32), 0.3, 6,
                             [9, 3, 7, -1, 9, 2])
    assert slots.tolist() == [2, 0] and values.tolist() == [np.float32(0.3) * np.float32(0.5)] * 2
    assert mmr_host([], np.zeros((0, 0)), 0.5, 4)[0].size == 0
    with pytest.raises(ValueError):
        mmr_host([0.1], np.zeros((1, 1)), 1.5, 1)


def test_lambda_one_is_the_sort_by_rel_then_id():
    rng = np.random.default_rng(3)
    for _ in range(50):
        n = int(rng.integers(1, 60))
        rel = rng.choice(np.asarray([-1.0, -0.0, 0.0, 0.25, 0.5, 0.75, 1.0], dtype=np.float32), size=n)
        ids = rng.permutation(500)[:n].astype(np.int64)
        cos = rng.uniform(-1, 1, size=(n, n)).astype(np.float32)
        k = int(rng.integers(1, n + 1))
        want = sorted(range(n), key=lambda i: (-float(rel[i]), int(ids[i])))[:k]
        slots, values = mmr_host(rel, cos, 1.0, k, ids)
        assert slots.tolist() == want and np.array_equal(values, rel[want])
        assert mmr_oracle(rel, cos, 1.0, k, ids)[0].tolist() == want


def test_params_record():
    assert MmrParams(0.5).fetch_for(10) == 40 and MmrParams(0.5).fetch_for(100) == 256
    assert MmrParams(0.5, fetch=30).fetch_for(10) == 30 and MmrParams(0.5, fetch=5).fetch_for(10) == 10
    assert MmrParams(0.0, fetch=1000).fetch_for(10) == 256
    for bad in (dict(lam=-0.1), dict(lam=1.1), dict(lam=float("nan")), dict(lam=0.5, fetch=-1)):
        with pytest.raises(ValueError):
            MmrParams(**bad)


C_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


def declared(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    ret, args = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text).groups()
    kinds = []
    for arg in args.split(","):
        arg = arg.strip()
        kinds.append(ctypes.c_void_p if "*" in arg else C_TYPES[arg.split()[-2]])
    return C_TYPES[ret], kinds


def test_binding_and_header_agree():
    text = HEADER.read_text()
    assert int(re.search(r"#define CRAG_MMR_MAX_WIDTH (\d+)", text).group(1)) == _native.CRAG_MMR_MAX_WIDTH == 256
    for name in ("crag_index_mmr_scratch_bytes", "crag_index_mmr_async"):
        restype, argtypes = _native.SIGNATURES[name]
        assert (restype, list(argtypes)) == declared(name), name
    assert len(_native.SIGNATURES["crag_index_mmr_async"][1]) == 17


def test_scratch_bytes(native_lib):
    fn = native_lib.crag_index_mmr_scratch_bytes
    nqs, widths = (1, 2, 3, 17, 64, 65535), (1, 2, 31, 32, 33, 64, 65, 255, 256)
    sizes = {(nq, w): int(fn(nq, w)) for nq in nqs for w in widths}
    for (nq, w), v in sizes.items():
        assert v > 0 and v % 8 == 0
        assert v >= nq * w * w * 4                                         # an fp32 cosine per (query, pair)
        assert all(v < sizes[(nq2, w)] for nq2 in nqs if nq2 > nq)
        assert all(v <= sizes[(nq, w2)] for w2 in widths if w2 > w)         # whole blocks of 32: 33 and 64 cost the same
        assert all(v < sizes[(nq, w2)] for w2 in widths if (w2 + 31) // 32 > (w + 31) // 32)


def test_argument_errors_are_codes_with_a_message(native_lib):
    """Checked before any HIP call: stand-in pointers are never dereferenced."""
    fn = native_lib.crag_index_mmr_async
    need = int(native_lib.crag_index_mmr_scratch_bytes(2, 40))
    some = np.zeros(64, dtype=np.uint64)
    P = some.ctypes.data

    def call(ix=P, ids=P, rel=P, counts=P, nq=2, width=40, lam=0.5, k=5, out_ids=P, out_rel=P, out_value=P, out_slots=P,
             out_sim_rows=P, out_counts=P, scratch=P, scratch_bytes=1 << 20):
        return fn(ix, ids, rel, counts, nq, width, lam, k, out_ids, out_rel, out_value, out_slots, out_sim_rows,
                  out_counts, scratch, scratch_bytes, None)

    bad = [dict(ix=None), dict(ids=None), dict(rel=None), dict(counts=None), dict(out_ids=None), dict(out_rel=None),
           dict(out_counts=None), dict(scratch=None), dict(nq=-1), dict(nq=65536), dict(width=0), dict(width=-3),
           dict(width=257), dict(k=0), dict(k=-1), dict(k=257), dict(lam=-0.01), dict(lam=1.01), dict(lam=float("nan")),
           dict(lam=float("inf")), dict(scratch_bytes=need - 1), dict(scratch_bytes=0), dict(scratch=P + 4),
           dict(nq=0, k=0), dict(nq=0, scratch=None), dict(nq=0, lam=2.0)]          # nq = 0 excuses nothing else
    for kw in bad:
        assert call(**kw) == -1, kw                # CRAG_EINVAL
        assert b"mmr" in native_lib.crag_last_error(), kw
    assert call(nq=0) == 0                         # nothing to do
    assert call(nq=0, out_value=None, out_slots=None, out_sim_rows=None, scratch_bytes=need, lam=1.0, k=256) == 0
    assert call(nq=0, width=256, scratch_bytes=int(native_lib.crag_index_mmr_scratch_bytes(0, 256))) == 0


def test_the_knob_is_read_and_off_by_default(monkeypatch):
    for name in ("DENSE_MMR_LAMBDA", "dense_mmr_lambda", "DENSE_MMR_FETCH", "dense_mmr_fetch"):
        monkeypatch.delenv(name, raising=False)
    assert Settings().dense_mmr_lambda == 1.0 and Settings.from_env().dense_mmr_lambda == 1.0
    assert Settings().dense_mmr_fetch == 0 and Settings.from_env().dense_mmr_fetch == 0
    monkeypatch.setenv("DENSE_MMR_LAMBDA", "0.6")
    monkeypatch.setenv("DENSE_MMR_FETCH", "120")
    assert Settings.from_env().dense_mmr_lambda == 0.6 and Settings.from_env().dense_mmr_fetch == 120
    monkeypatch.setattr(settings, "dense_mmr_fetch", 0)
    for value, want in ((1.0, None), (1.5, None), (float("nan"), None), (0.5, 0.5), (0.0, 0.0), (-2.0, 0.0)):
        monkeypatch.setattr(settings, "dense_mmr_lambda", value)
        got = rt._dense_mmr()
        assert (got is None) if want is None else (got == MmrParams(lam=want, fetch=0))
    monkeypatch.setattr(settings, "dense_mmr_fetch", 99)
    assert rt._dense_mmr() == MmrParams(lam=0.0, fetch=99)


def test_notes_carry_the_knob_only_when_it_is_on(monkeypatch):
    monkeypatch.setattr(settings, "embeddings_base_url", "")
    request = rt.RetrieveRequest(query="why did the renewal slip")
    monkeypatch.setattr(settings, "dense_mmr_lambda", 1.0)
    off = rt.retrieve_evidence(request, backend=rt.RetrieveBackend())
    assert "dense_mmr_lambda" not in off["notes"]["retrieval"]
    monkeypatch.setattr(settings, "dense_mmr_lambda", 0.5)
    on = rt.retrieve_evidence(request, backend=rt.RetrieveBackend())
    assert on["notes"]["retrieval"]["dense_mmr_lambda"] == 0.5
    del on["notes"]["retrieval"]["dense_mmr_lambda"]
    on.pop("query_id"), off.pop("query_id")
    assert on == off                               # nothing else changed
