"""The grouped search, host side (no GPU): the two forms of its contract -- the walk over the ranking and the top-k of the
union of per-group top-g -- agree in numpy; the binding and the header agree; the scratch is sized sensibly; every bad
argument is refused with a code and a message before a device is touched; the DENSE_PER_CALL_CAP knob is read, defaults to
off, and an unset knob leaves the retrieval notes as they were."""
import ctypes
import re
from pathlib import Path

import numpy as np

from cadence_rag_amd import _native
from cadence_rag_amd import retrieve as rt
from cadence_rag_amd.config import Settings, settings
from group_oracle import capped_topk, orderable, union_topk

HEADER = Path(__file__).resolve().parent.parent / "include" / "crag_dense.h"


def same(a, b):
    return (a[3] == b[3] and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
            and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))


def test_the_two_oracle_forms_agree():
    rng = np.random.default_rng(12)
    some_cut = False
    for case in range(200):
        n = int(rng.integers(1, 90))
        n_groups = int(rng.integers(1, 12))
        # few distinct scores: ties inside and across groups; -0.0 and +0.0 among them
        scores = rng.choice(np.asarray([-1.0, -0.5, -0.0, 0.0, 0.25, 0.5, 1.0], dtype=np.float32), size=n)
        ids = np.sort(rng.choice(1000, size=n, replace=False)).astype(np.int64)
        groups = rng.integers(-1, n_groups + 2, size=n).astype(np.int32)      # -1, n_groups and n_groups + 1 are out of range
        if n_groups > 1:                                                      # an empty group
            empty = int(rng.integers(0, n_groups))
            groups[groups == empty] = (empty + 1) % n_groups
        eligible = rng.random(n) < 0.8
        for k in (1, 3, 32, 128):
            for g in (1, 2, 3, 8):
                a = capped_topk(scores, ids, groups, eligible, k, g, n_groups)
                b = union_topk(scores, ids, groups, eligible, k, g, n_groups)
                assert same(a, b), (case, k, g)
                n_out = a[3]
                in_range = eligible & (groups >= 0) & (groups < n_groups)
                assert n_out <= min(k, int(in_range.sum()))
                assert (a[0][n_out:] == -1).all() and np.isnan(a[1][n_out:]).all() and (a[2][n_out:] == -1).all()
                assert ((a[2][:n_out] >= 0) & (a[2][:n_out] < n_groups)).all()
                assert n_out == 0 or np.bincount(a[2][:n_out]).max() <= g
                key = orderable(a[1][:n_out]).astype(np.int64)
                assert all((key[i], -a[0][i]) > (key[i + 1], -a[0][i + 1]) for i in range(n_out - 1))
                some_cut = some_cut or n_out < min(k, int(in_range.sum()))
    assert some_cut   # the cap did leave rows out somewhere


def test_the_oracle_on_a_case_by_hand():
    scores = np.asarray([0.9, 0.9, 0.8, 0.7, 0.6, 0.5], dtype=np.float32)
    ids = np.asarray([5, 3, 9, 11, 12, 20], dtype=np.int64)
    groups = np.asarray([0, 0, 0, 1, 7, -1], dtype=np.int32)
    everyone = np.ones(6, dtype=bool)
    got = capped_topk(scores, ids, groups, everyone, 4, 2, n_groups=7)    # group 7 and -1 are out of range
    assert got[3] == 3 and got[0].tolist() == [3, 5, 11, -1] and got[2].tolist() == [0, 0, 1, -1]
    got = capped_topk(scores, ids, groups, everyone, 4, 1, n_groups=8)
    assert got[3] == 3 and got[0].tolist() == [3, 11, 12, -1]


C_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64}


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
    assert int(re.search(r"#define CRAG_GROUP_MAX_PER (\d+)", text).group(1)) == _native.CRAG_GROUP_MAX_PER == 8
    for name in ("crag_index_search_grouped_scratch_bytes", "crag_index_search_grouped_async"):
        restype, argtypes = _native.SIGNATURES[name]
        assert (restype, list(argtypes)) == declared(name), name
    assert len(_native.SIGNATURES["crag_index_search_grouped_async"][1]) == 16


def test_scratch_bytes(native_lib):
    fn = native_lib.crag_index_search_grouped_scratch_bytes
    nqs, ngs, pers = (1, 2, 3, 17, 64, 65535), (1, 2, 23, 2000, (1 << 31) - 1), (1, 2, 3, 8)
    sizes = {(nq, ng, g): int(fn(nq, ng, g)) for nq in nqs for ng in ngs for g in pers}
    for (nq, ng, g), v in sizes.items():
        assert v > 0 and v % 8 == 0
        assert v >= nq * ng * g * 8                                        # a 64-bit key per (query, group, slot)
        assert all(v < sizes[(nq2, ng, g)] for nq2 in nqs if nq2 > nq)
        assert all(v < sizes[(nq, ng2, g)] for ng2 in ngs if ng2 > ng)
        assert all(v < sizes[(nq, ng, g2)] for g2 in pers if g2 > g)


def test_argument_errors_are_codes_with_a_message(native_lib):
    """Checked before any HIP call: stand-in pointers are never dereferenced."""
    fn = native_lib.crag_index_search_grouped_async
    need = int(native_lib.crag_index_search_grouped_scratch_bytes(2, 23, 2))
    some = np.zeros(64, dtype=np.uint64)
    P = some.ctypes.data

    def call(ix=P, queries=P, nq=2, k=5, row_group=P, n_groups=23, per_group=2, mask=None, stride=0, out_ids=P,
             out_scores=P, out_groups=P, out_counts=P, scratch=P, scratch_bytes=1 << 20):
        return fn(ix, queries, nq, k, row_group, n_groups, per_group, mask, stride, out_ids, out_scores, out_groups,
                  out_counts, scratch, scratch_bytes, None)

    bad = [dict(ix=None), dict(queries=None), dict(row_group=None), dict(out_ids=None), dict(out_scores=None),
           dict(out_counts=None), dict(scratch=None), dict(nq=-1), dict(nq=65536), dict(k=0), dict(k=-3), dict(k=129),
           dict(per_group=0), dict(per_group=-1), dict(per_group=9), dict(n_groups=0), dict(n_groups=-4),
           dict(n_groups=1 << 31), dict(n_groups=1 << 40), dict(mask=P, stride=6), dict(mask=P, stride=-4),
           dict(mask=P + 2, stride=0), dict(scratch_bytes=need - 1), dict(scratch_bytes=0), dict(scratch=P + 4),
           dict(nq=0, k=0), dict(nq=0, scratch=None)]                         # nq = 0 excuses nothing else
    for kw in bad:
        assert call(**kw) == -1, kw                # CRAG_EINVAL
        assert b"search_grouped" in native_lib.crag_last_error(), kw
    assert call(nq=0) == 0                         # nothing to do
    assert call(nq=0, out_groups=None, mask=P, stride=8, scratch_bytes=need) == 0


def test_the_knob_is_read_and_off_by_default(monkeypatch):
    monkeypatch.delenv("DENSE_PER_CALL_CAP", raising=False)
    monkeypatch.delenv("dense_per_call_cap", raising=False)
    assert Settings().dense_per_call_cap == 0 and Settings.from_env().dense_per_call_cap == 0
    monkeypatch.setenv("DENSE_PER_CALL_CAP", "3")
    assert Settings.from_env().dense_per_call_cap == 3
    for value, want in ((0, 0), (-2, 0), (2, 2), (8, 8), (50, _native.CRAG_GROUP_MAX_PER)):
        monkeypatch.setattr(settings, "dense_per_call_cap", value)
        assert rt._dense_per_call_cap() == want


def test_notes_carry_the_cap_only_when_it_is_on(monkeypatch):
    monkeypatch.setattr(settings, "embeddings_base_url", "")
    request = rt.RetrieveRequest(query="why did the renewal slip")
    monkeypatch.setattr(settings, "dense_per_call_cap", 0)
    off = rt.retrieve_evidence(request, backend=rt.RetrieveBackend())
    assert "dense_per_call_cap" not in off["notes"]["retrieval"]
    monkeypatch.setattr(settings, "dense_per_call_cap", 2)
    on = rt.retrieve_evidence(request, backend=rt.RetrieveBackend())
    assert on["notes"]["retrieval"]["dense_per_call_cap"] == 2
    del on["notes"]["retrieval"]["dense_per_call_cap"]
    on.pop("query_id"), off.pop("query_id")
    assert on == off                               # nothing else changed
