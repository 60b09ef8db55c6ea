"""Sampling on the host: the Philox known answers, the uniform's range, sample_host on hand cases, the argument checks of
crag_enc_sample and crag_enc_grammar_advance (they come before anything is enqueued, so they hold without a GPU), the
binding against the header, and /answer's request fields."""
from __future__ import annotations

import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

from cadence_rag_amd import _native, answer, grammar, retrieve, sampling
from cadence_rag_amd.answer import AnswerRequest
from cadence_rag_amd.config import settings
from cadence_rag_amd.sampling import SamplingParams, min_p_cut, philox4x32_10, philox_uniform_host, sample_host

HEADER = Path(__file__).resolve().parent.parent / "include" / "crag_encoder.h"


# ---- Philox -----------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds."""
    zero = philox4x32_10((0, 0, 0, 0), (0, 0))[0]
    assert [f"{int(x):08x}" for x in zero] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    ones = philox4x32_10((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2)[0]
    assert [f"{int(x):08x}" for x in ones] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    pi = philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))[0]
    assert [f"{int(x):08x}" for x in pi] == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]


def test_philox_is_vectorised_over_the_token_id():
    ids = np.array([0, 1, 77, 151935, 2 ** 31 - 1])
    rows = philox4x32_10((ids, 5, 3, 0), (11, 12))
    for i, row in zip(ids, rows):
        assert np.array_equal(row, philox4x32_10((int(i), 5, 3, 0), (11, 12))[0])
    assert len({tuple(r) for r in rows.tolist()}) == len(ids)


def test_uniform_lies_strictly_inside_the_unit_interval():
    u = philox_uniform_host(seed=2 ** 63 + 5, step=9, stream=2, ids=np.arange(200_000))
    assert u.min() > 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.01
    # the ends of the formula itself: x0 = 0 and x0 = 2^32 - 1
    assert (0 + 0.5) * 2.0 ** -24 > 0.0 and ((0xFFFFFFFF >> 8) + 0.5) * 2.0 ** -24 < 1.0
    assert np.isfinite(-np.log(-np.log(u))).all()
    # the seed's two halves are the key; step and stream are counter words
    a = philox_uniform_host(1, 0, 0, [4])[0]
    assert len({a, philox_uniform_host(1 << 32, 0, 0, [4])[0], philox_uniform_host(1, 1, 0, [4])[0],
                philox_uniform_host(1, 0, 1, [4])[0]}) == 4


# ---- the rule ---------------------------------------------------------------------------------------------------------
def _row(n=300, seed=0):
    return (np.random.default_rng(seed).standard_normal(n) * 3).astype(np.float32)


def test_parameters_are_range_checked():
    for bad in (dict(temperature=-1), dict(temperature=0.001), dict(temperature=101), dict(temperature=math.nan),
                dict(temperature=1, top_k=-1), dict(temperature=1, top_k=1.5), dict(temperature=1, top_p=0),
                dict(temperature=1, top_p=1.01), dict(temperature=1, min_p=-0.1), dict(temperature=1, min_p=1.1),
                dict(temperature=1, seed=-1), dict(temperature=1, seed=2 ** 64)):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    p = SamplingParams(0.7, top_k=5, top_p=0.9, min_p=0.1, seed=2 ** 64 - 1)
    assert p.echo() == {"temperature": 0.7, "top_k": 5, "top_p": 0.9, "min_p": 0.1, "seed": 2 ** 64 - 1} and not p.greedy
    assert SamplingParams(0).greedy
    assert min_p_cut(0.7, 0) == -np.inf and min_p_cut(0.7, 1) == 0 and min_p_cut(0.0, 0.5) == 0
    assert min_p_cut(2.0, 0.05) == np.float32(float(np.float32(2.0)) * math.log(0.05))
    with pytest.raises(ValueError):
        sample_host(_row(10), SamplingParams(1.0, top_k=11), 0, 0)


def test_greedy_forms_give_the_greedy_token():
    row = _row()
    row[[17, 40]] = row.max() + 1            # a tie at the top: a greedy row takes the lowest id
    got = sample_host(row, SamplingParams(0.0), 3, 1)
    assert (got.token, got.kept, got.cut) == (17, 2, float(row[17]))
    assert sample_host(row, SamplingParams(1.0, top_k=1), 3, 1).kept == 2      # a cut keeps the tie together
    row[40] -= 0.5
    for step in range(5):
        for params in (SamplingParams(0.0), SamplingParams(1.0, top_p=1e-6, seed=step), SamplingParams(0.01, top_p=1e-6),
                       SamplingParams(1.0, top_k=1, seed=step)):
            got = sample_host(row, params, step, 1)
            assert (got.token, got.kept, got.cut) == (17, 1, float(row[17]))


def test_min_p_one_keeps_exactly_the_maxima():
    row = _row()
    row[[5, 99, 250]] = row.max() + 2
    seen = set()
    for step in range(40):
        got = sample_host(row, SamplingParams(1.0, min_p=1.0, seed=3), step, 0)
        assert got.kept == 3 and got.cut == float(row[5])
        seen.add(got.token)
    assert seen == {5, 99, 250}              # and the draw is among them: each turns up within 40 steps


def test_two_levels_keep_exactly_the_high_tokens():
    row = np.full(64, -4.0, np.float32)
    high = [3, 20, 21, 63]
    row[high] = 6.0                          # e^10 between the levels: the four hold 0.9997 of the mass
    for params, kept in ((SamplingParams(1.0, top_p=0.9), 4), (SamplingParams(1.0, top_k=2), 4),   # ties stay together
                         (SamplingParams(1.0, top_k=5), 64), (SamplingParams(1.0, min_p=0.01), 4),
                         (SamplingParams(1.0, top_p=0.9999), 64), (SamplingParams(1.0), 64)):
        got = sample_host(row, params, 0, 0)
        assert got.kept == kept and got.cut == (6.0 if kept == 4 else -4.0), params
        assert kept == 64 or got.token in high
    counts = np.zeros(64, int)
    for step in range(400):
        counts[sample_host(row, SamplingParams(1.0, top_p=0.9, seed=5), step, 0).token] += 1
    assert counts[high].sum() == 400 and counts[high].min() > 60      # four equal weights: 100 each, sd 8.7


def test_candidates_and_special_values():
    row = _row(40)
    allowed = np.zeros(40, bool)
    allowed[[7, 8, 30]] = True
    row[7], row[8] = np.nan, -np.inf
    assert sample_host(row, SamplingParams(1.0), 0, 0, allowed=allowed)[:3] == (30, math.inf, 1)
    allowed[30] = False
    got = sample_host(row, SamplingParams(1.0), 0, 0, allowed=allowed)
    assert (got.token, got.kept) == (-1, 0) and math.isnan(got.cut)
    row[[12, 33]] = np.inf
    got = sample_host(row, SamplingParams(1.0, top_k=1), 0, 0)
    assert (got.token, got.kept, got.cut) == (12, 2, math.inf)
    # -0 and +0 are one logit value
    zeros = np.array([-1.0, -0.0, 0.0, -2.0], np.float32)
    assert sample_host(zeros, SamplingParams(1.0, top_k=1), 0, 0).kept == 2
    assert sample_host(zeros, SamplingParams(0.0), 0, 0).token == 1


def test_the_delta_band_brackets_the_count():
    row = _row(2000, seed=4)
    for step in range(20):
        got = sample_host(row, SamplingParams(0.7, top_p=0.9, seed=1), step, 0)
        assert got.kept_lo <= got.kept <= got.kept_hi and 0 < got.kept < 2000
        assert got.gap >= 0 and got.cut == np.sort(row)[::-1][got.kept - 1]


# ---- the C entries' argument checks ------------------------------------------------------------------------------------
def test_sample_argument_errors_are_codes(native_lib):
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = lambda *v: (ctypes.c_float * 8)(*v)      # noqa: E731
    i = lambda *v: (ctypes.c_int32 * 8)(*v)      # noqa: E731
    u = lambda *v: (ctypes.c_uint32 * 8)(*v)     # noqa: E731
    names = ["logits", "vocab", "allowed_bits", "temperature", "top_k", "top_p", "min_p_cut", "stream", "seed", "step",
             "token", "kept", "cut", "n_rows", "hip_stream"]
    good = [p, 100, None, f(1.0, 0.0), i(0, 0), f(1.0, 1.0), f(-math.inf, 0.0), u(0, 1), 7, 0, p, None, None, 2, None]

    def call(**change):
        args = list(good)
        for k, v in change.items():
            args[names.index(k)] = v
        return native_lib.crag_enc_sample(*args)

    for name in ("logits", "temperature", "top_k", "top_p", "min_p_cut", "stream", "token"):
        assert call(**{name: None}) == -1 and "NULL" in _native.last_error(), name
    off = lambda k: ctypes.c_void_p(p.value + k)   # noqa: E731
    for change, word in (({"n_rows": 0}, "n_rows"), ({"n_rows": _native.CRAG_DECODE_MAX_SEQS + 1}, "n_rows"),
                         ({"vocab": 0}, "vocab"), ({"vocab": -1}, "vocab"), ({"vocab": 2 ** 31}, "vocab"),
                         ({"temperature": f(1.0, -1.0)}, "temperature"), ({"temperature": f(0.009, 0.0)}, "temperature"),
                         ({"temperature": f(1.0, 100.5)}, "temperature"), ({"temperature": f(math.nan, 0.0)}, "temperature"),
                         ({"top_k": i(0, -1)}, "top_k"), ({"top_k": i(101, 0)}, "top_k"),
                         ({"top_p": f(0.0, 1.0)}, "top_p"), ({"top_p": f(1.0, 1.5)}, "top_p"),
                         ({"top_p": f(math.nan, 1.0)}, "top_p"), ({"min_p_cut": f(0.5, 0.0)}, "min_p_cut"),
                         ({"min_p_cut": f(0.0, math.nan)}, "min_p_cut"),
                         ({"logits": off(2)}, "aligned"), ({"token": off(1)}, "aligned"), ({"kept": off(2)}, "aligned"),
                         ({"cut": off(3)}, "aligned"), ({"allowed_bits": off(2)}, "aligned")):
        assert call(**change) == -1 and word in _native.last_error(), (change, _native.last_error())
    assert (_native.CRAG_SAMPLE_MIN_TEMPERATURE, _native.CRAG_SAMPLE_MAX_TEMPERATURE) == \
        (sampling.MIN_TEMPERATURE, sampling.MAX_TEMPERATURE)


def test_grammar_advance_argument_errors_are_codes(native_lib):
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    names = ["tok_offsets", "tok_bytes", "tok_kind", "vocab", "class_of", "trans", "n_states", "n_classes", "state", "token",
             "n_rows", "stream"]
    good = [p, p, p, 100, p, p, 4, 4, p, p, 1, None]

    def call(**change):
        args = list(good)
        for k, v in change.items():
            args[names.index(k)] = v
        return native_lib.crag_enc_grammar_advance(*args)

    for name in ("tok_offsets", "tok_bytes", "tok_kind", "class_of", "trans", "state", "token"):
        assert call(**{name: None}) == -1 and "NULL" in _native.last_error(), name
    for change, word in (({"n_rows": 0}, "n_rows"), ({"n_rows": _native.CRAG_DECODE_MAX_SEQS + 1}, "n_rows"),
                         ({"n_states": 0}, "n_states"), ({"n_states": grammar.MAX_STATES + 1}, "n_states"),
                         ({"n_classes": 0}, "n_classes"), ({"n_classes": grammar.MAX_CLASSES + 1}, "n_classes"),
                         ({"vocab": 0}, "vocab"), ({"vocab": 2 ** 31}, "vocab"),
                         ({"trans": ctypes.c_void_p(p.value + 1)}, "aligned"),
                         ({"state": ctypes.c_void_p(p.value + 2)}, "aligned"),
                         ({"token": ctypes.c_void_p(p.value + 2)}, "aligned")):
        assert call(**change) == -1 and word in _native.last_error(), (change, _native.last_error())


# ---- binding == header -------------------------------------------------------------------------------------------------
_CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32,
           "float": ctypes.c_float}


def _declared(name: str):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    ret, args = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text).groups()
    types = []
    for arg in args.split(","):
        arg = arg.strip()
        types.append(ctypes.c_void_p if "*" in arg else _CTYPES[arg.replace("const ", "").split()[0]])
    return _CTYPES[ret], types


@pytest.mark.parametrize("name", ["crag_enc_sample", "crag_enc_grammar_advance"])
def test_binding_equals_header(native_lib, name):
    restype, argtypes = _native.SIGNATURES[name]
    assert (restype, argtypes) == _declared(name)
    assert hasattr(native_lib, name)
    text = HEADER.read_text()
    assert float(re.search(r"#define CRAG_SAMPLE_MIN_TEMPERATURE ([0-9.]+)f", text).group(1)) == \
        _native.CRAG_SAMPLE_MIN_TEMPERATURE
    assert float(re.search(r"#define CRAG_SAMPLE_MAX_TEMPERATURE ([0-9.]+)f", text).group(1)) == \
        _native.CRAG_SAMPLE_MAX_TEMPERATURE


# ---- /answer ------------------------------------------------------------------------------------------------------------
def _items(n):
    return [{"evidence_id": f"Q-{10 + i}", "call_id": f"call-{i % 2}", "chunk_id": 10 + i, "speaker": "agent",
             "start_ts_ms": 0, "end_ts_ms": 1, "snippet": f"fact number {i}", "why_relevant": "bm25"} for i in range(n)]


@pytest.fixture
def pack(monkeypatch):
    def fake(request, backend=None):
        return {"query_id": "00000000-0000-0000-0000-000000000001", "intent": request.intent, "budget": {},
                "artifacts": [], "quotes": _items(3), "notes": {}}

    monkeypatch.setattr(retrieve, "retrieve_evidence", fake)
    monkeypatch.setattr(settings, "answer_max_repairs", 1)
    yield
    answer.set_llm(None)


@pytest.fixture
def http(pack, monkeypatch):
    bodies = []

    def post(url, headers, body, timeout_s):
        bodies.append(body)
        return 200, '{"choices": [{"message": {"content": "The fact holds [Q-10]."}}], "model": "m"}'

    monkeypatch.setattr(settings, "llm_base_url", "http://llm.invalid/v1")
    monkeypatch.setattr(answer, "_post_json", post)
    return bodies


def test_settings_default_to_greedy(monkeypatch):
    s = type(settings).from_env()
    assert (s.answer_temperature, s.answer_top_p, s.answer_top_k, s.answer_min_p, s.answer_seed) == (0.0, 1.0, 0, 0.0, 0)
    monkeypatch.setenv("ANSWER_TEMPERATURE", "0.6")
    monkeypatch.setenv("ANSWER_SEED", "12")
    s = type(settings).from_env()
    assert (s.answer_temperature, s.answer_seed) == (0.6, 12)
    request = AnswerRequest(query="q")
    assert (request.temperature, request.top_p, request.top_k, request.min_p, request.seed) == (None,) * 5
    assert answer.sampling_for(request) is None


def test_request_defaults_leave_the_http_body_and_the_notes_unchanged(http):
    out = answer.answer_question(AnswerRequest(query="what holds?"))
    assert out["status"] == "ok"
    (body,) = http
    assert sorted(body) == ["max_tokens", "messages", "model", "temperature"] and body["temperature"] == 0
    assert sorted(out["notes"]) == ["dropped_evidence", "evidence_items", "llm_calls", "validator"]


def test_request_fields_reach_the_http_body_and_the_notes(http, monkeypatch):
    out = answer.answer_question(AnswerRequest(query="what holds?", temperature=0.7, seed=9))
    (body,) = http
    assert (body["temperature"], body["top_p"], body["seed"]) == (0.7, 1.0, 9)
    assert sorted(body) == ["max_tokens", "messages", "model", "seed", "temperature", "top_p"]
    assert out["notes"]["sampling"] == {"temperature": 0.7, "top_k": 0, "top_p": 1.0, "min_p": 0.0, "seed": 9}
    # a field alone, at temperature 0, is still a request for these parameters
    out = answer.answer_question(AnswerRequest(query="what holds?", top_p=0.5))
    assert http[1]["top_p"] == 0.5 and http[1]["temperature"] == 0.0 and out["notes"]["sampling"]["top_p"] == 0.5
    # the settings are the defaults under the request
    monkeypatch.setattr(settings, "answer_temperature", 0.3)
    monkeypatch.setattr(settings, "answer_top_k", 40)
    out = answer.answer_question(AnswerRequest(query="what holds?", seed=2))
    assert out["notes"]["sampling"] == {"temperature": 0.3, "top_k": 40, "top_p": 1.0, "min_p": 0.0, "seed": 2}
    with pytest.raises(answer.AnswerRequestError):
        answer.answer_question(AnswerRequest(query="what holds?", temperature=1000.0))


class _Sampler:
    model_id = "stub"
    supports_sampling = True

    def __init__(self, replies):
        self.calls, self.replies = [], list(replies)

    def generate_text(self, messages, max_new_tokens, **kw):
        self.calls.append(kw)
        return self.replies.pop(0)


class _Greedy:
    model_id = "stub"

    def __init__(self):
        self.calls = 0

    def generate_text(self, messages, max_new_tokens):
        self.calls += 1
        return "The fact holds [Q-10]."


def test_native_model_gets_the_parameters_and_a_stream_per_attempt(pack, monkeypatch):
    monkeypatch.setattr(settings, "llm_base_url", "native")
    llm = _Sampler(["An uncited claim.", "The fact holds [Q-10]."])
    answer.set_llm(llm)
    out = answer.answer_question(AnswerRequest(query="what holds?", temperature=0.8, top_k=20, seed=4))
    want = SamplingParams(0.8, top_k=20, seed=4)
    assert out["status"] == "ok" and out["repairs"] == 1 and out["notes"]["sampling"] == want.echo()
    assert llm.calls == [{"sampling": want, "stream": 0}, {"sampling": want, "stream": 1}]
    # without sampling the model is called as ever: no keyword at all
    llm = _Sampler(["The fact holds [Q-10]."])
    answer.set_llm(llm)
    out = answer.answer_question(AnswerRequest(query="what holds?"))
    assert llm.calls == [{}] and "sampling" not in out["notes"]
    # a model that cannot sample is not handed the keyword, and the notes say so
    plain = _Greedy()
    answer.set_llm(plain)
    out = answer.answer_question(AnswerRequest(query="what holds?", temperature=0.8))
    assert out["status"] == "ok" and plain.calls == 1 and out["notes"]["sampling"]["applied"] is False
