"""The search plan, host side (no GPU): which kernels a dense search takes and how it sizes them is a pure function of
(size, n_cu, nq, k, mirror, irregular, developer switches).  crag_search_plan_ hands that function out; every field is
compared with a transcription of the dispatch rules, over every class boundary of nq, k and size, and a few rows are
written out by hand."""
import ctypes as C
import itertools

import pytest

from cadence_rag_amd import _native

FIELDS = ("wide", "q_blocks", "nq_pad", "G", "prefilter", "cap", "rsplit", "nb", "pub_rank", "sets", "pub0",
          "derive_lag", "read_lag", "nt", "fb_blocks", "window_too_large")

DIM, GB_CELLS, PF_MIN_ROWS_PER_GROUP = 1024, 32, 128
DEFAULTS = dict(no_wide=0, no_prefilter=0, no_rsplit=0, derive_lag=2, read_lag=4, pf_nt=-1, nt_above_bytes=1536 << 20)


class Plan(C.Structure):
    _fields_ = [(name, C.c_int32) for name in FIELDS]


@pytest.fixture(scope="module")
def hook():
    fn = _native.load().crag_search_plan_
    fn.restype = C.c_int
    fn.argtypes = [C.c_int64] + [C.c_int] * 11 + [C.c_int64, C.POINTER(Plan)]
    return fn


def native_plan(hook, size, n_cu, nq, k, mirror, irregular, **switches):
    sw = dict(DEFAULTS, **switches)
    out = Plan()
    n = hook(size, n_cu, nq, k, int(mirror), int(irregular), sw["no_wide"], sw["no_prefilter"], sw["no_rsplit"],
             sw["derive_lag"], sw["read_lag"], sw["pf_nt"], sw["nt_above_bytes"], C.byref(out))
    assert n == C.sizeof(Plan)
    return {name: getattr(out, name) for name in FIELDS}


def ceil_div(a, b):
    return -(-a // b)


def expected_plan(size, n_cu, nq, k, mirror, irregular, **switches):
    """The dispatch rules, transcribed from the search's launch sequence as it stood before the plan existed."""
    sw = dict(DEFAULTS, **switches)
    p = {}
    wide = nq > 32 and not sw["no_wide"]
    p["wide"] = int(wide)
    p["q_blocks"] = ceil_div(nq, 64) * 2 if wide else ceil_div(nq, 32)
    p["nq_pad"] = p["q_blocks"] * 32
    G = p["G"] = max(1, min(n_cu, ceil_div(size, 8)))
    p["prefilter"] = int(not sw["no_prefilter"] and not irregular and size >= G * PF_MIN_ROWS_PER_GROUP
                         and (wide or nq <= 32))
    p["cap"] = 32768 if (k > 104 and p["nq_pad"] <= 128) else 8192
    p["rsplit"] = 1 if (k <= 32 or sw["no_rsplit"]) else 8 if nq <= 16 else 4 if nq <= 128 else 1
    p["nb"] = min(k, GB_CELLS)
    p["pub_rank"] = ceil_div(k, p["nb"]) - 1
    p["sets"] = 1 if k <= 24 else 2 if k <= 56 else 4
    p["pub0"] = 8 if ceil_div(k, p["sets"]) >= 27 else p["sets"]
    p["derive_lag"] = sw["derive_lag"] if mirror else 1
    p["read_lag"] = sw["read_lag"] if mirror else 2
    if not mirror:
        p["nt"] = 0
    elif sw["pf_nt"] >= 0:
        p["nt"] = sw["pf_nt"]
    else:
        p["nt"] = int(size * DIM * 2 > sw["nt_above_bytes"])
    p["fb_blocks"] = G * ceil_div(nq, 32)
    p["window_too_large"] = int((ceil_div(size, G) + 64) * DIM * 4 >= 0x7FF00000)
    return p


NQS = (1, 16, 17, 32, 33, 64, 65, 128, 129)
KS = (1, 24, 25, 32, 33, 56, 57, 104, 105, 128)


def sizes(n_cu):
    return (0, 7, 8, 128 * n_cu - 1, 128 * n_cu, 1_000_000)


@pytest.mark.parametrize("n_cu", [256, 4])
def test_plan_matches_the_dispatch_rules(hook, n_cu):
    seen = {name: set() for name in FIELDS}
    for nq, k, size, mirror, irregular in itertools.product(NQS, KS, sizes(n_cu), (True, False), (False, True)):
        got = native_plan(hook, size, n_cu, nq, k, mirror, irregular)
        assert got == expected_plan(size, n_cu, nq, k, mirror, irregular), (size, n_cu, nq, k, mirror, irregular)
        for name in FIELDS:
            seen[name].add(got[name])
    # the product reaches both sides of every decision (the window limit has a test of its own)
    assert seen["wide"] == {0, 1} and seen["prefilter"] == {0, 1} and seen["nt"] == {0, 1}
    assert seen["cap"] == {8192, 32768} and seen["rsplit"] == {1, 4, 8} and seen["sets"] == {1, 2, 4}
    assert seen["pub0"] == {1, 2, 4, 8} and seen["derive_lag"] == {1, 2} and seen["read_lag"] == {2, 4}


SWITCHES = [dict(no_wide=1), dict(no_prefilter=1), dict(no_rsplit=1), dict(derive_lag=1, read_lag=3),
            dict(derive_lag=1, read_lag=2), dict(pf_nt=0), dict(pf_nt=1), dict(nt_above_bytes=0),
            dict(nt_above_bytes=1 << 40)]


@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: ",".join(f"{k}={v}" for k, v in s.items()))
def test_each_developer_switch_alone(hook, switch):
    changed = False
    for nq, k, size, mirror in itertools.product(NQS, KS, sizes(256), (True, False)):
        got = native_plan(hook, size, 256, nq, k, mirror, False, **switch)
        assert got == expected_plan(size, 256, nq, k, mirror, False, **switch), (size, nq, k, mirror, switch)
        changed = changed or got != native_plan(hook, size, 256, nq, k, mirror, False)
    assert changed, "the switch reaches the plan"


def test_switches_do_not_come_from_the_environment(hook, monkeypatch):
    before = native_plan(hook, 100_000, 256, 64, 50, True, False)
    for name in ("CRAG_NO_WIDE", "CRAG_NO_PREFILTER", "CRAG_NO_RSPLIT", "CRAG_PF_NT"):
        monkeypatch.setenv(name, "1")
    monkeypatch.setenv("CRAG_PF_LAGS", "1,2")
    assert native_plan(hook, 100_000, 256, 64, 50, True, False) == before


def test_anchor_rows(hook):
    # the benchmark's shape: 100 000 rows x 64 queries, k = 10, on 256 CUs
    p = native_plan(hook, 100_000, 256, 64, 10, True, False)
    assert p == dict(wide=1, q_blocks=2, nq_pad=64, G=256, prefilter=1, cap=8192, rsplit=1, nb=10, pub_rank=0, sets=1,
                     pub0=1, derive_lag=2, read_lag=4, nt=0, fb_blocks=512, window_too_large=0)
    p = native_plan(hook, 100_000, 256, 64, 50, True, False)
    assert (p["sets"], p["pub0"], p["rsplit"], p["cap"], p["nb"], p["pub_rank"]) == (2, 2, 4, 8192, 32, 1)
    p = native_plan(hook, 100_000, 256, 8, 100, True, False)
    assert (p["wide"], p["q_blocks"], p["sets"], p["pub0"], p["rsplit"], p["cap"]) == (0, 1, 4, 4, 8, 8192)
    p = native_plan(hook, 100_000, 256, 64, 128, True, False)
    assert (p["cap"], p["sets"], p["pub0"], p["rsplit"], p["pub_rank"]) == (32768, 4, 8, 4, 3)
    # k = 128 with more than 128 padded queries: the candidate lists stay short
    assert native_plan(hook, 100_000, 256, 129, 128, True, False)["cap"] == 8192
    # 33 .. 64 queries without the wide kernels: no prefilter scan for them
    p = native_plan(hook, 100_000, 256, 33, 10, True, False, no_wide=1)
    assert (p["wide"], p["q_blocks"], p["prefilter"]) == (0, 2, 0)
    # a small corpus: one workgroup per 8 rows, the plain fp32 scan
    p = native_plan(hook, 20, 256, 1, 10, True, False)
    assert (p["G"], p["prefilter"], p["fb_blocks"]) == (3, 0, 3)
    # 1M rows: the mirror (2 GB) streams; without it there is nothing to stream and the lags are the fp32 scan's
    assert native_plan(hook, 1_000_000, 256, 64, 10, True, False)["nt"] == 1
    p = native_plan(hook, 1_000_000, 256, 64, 10, False, False)
    assert (p["nt"], p["derive_lag"], p["read_lag"], p["prefilter"]) == (0, 1, 2, 1)


def test_window_limit(hook):
    # 4 workgroups: a window of 523 968 + 64 rows x 4 KiB is exactly 0x7ff00000 bytes
    size = 4 * 523_968
    assert native_plan(hook, size, 4, 1, 10, True, False)["window_too_large"] == 1
    assert native_plan(hook, size - 4, 4, 1, 10, True, False)["window_too_large"] == 0
    for s in (size, size - 4):
        assert native_plan(hook, s, 4, 1, 10, True, False) == expected_plan(s, 4, 1, 10, True, False)
