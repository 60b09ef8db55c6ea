"""Constrained decoding for /answer: a deterministic byte automaton, the citation grammar built from an evidence pack,
the byte table of a tokenizer's vocabulary, and the host rule for which tokens a state allows.

  ByteDfa            class_of uint8[256], trans uint16[n_states, n_classes] (DEAD = 0xFFFF), accept uint8[n_states], start
  citation_grammar   "every sentence is cited, every id is in the pack" as a ByteDfa (sound against
                     answer.validate_citations: what it accepts is valid; some valid answers are refused)
  TokenTable         the raw bytes of every token id (offsets / bytes) and its kind: 0 ordinary, 1 stop, 2 never allowed
  TokenGrammar       (dfa, table): what Qwen3Generator.generate(grammar=...) takes
  walk / allowed_tokens_host / next_state_host
                     the rule crag_enc_grammar_argmax (csrc/crag_grammar.hip) implements, in numpy: the tests' oracle

The citation grammar.  A state is (sentence, position, flag) plus what is being read:
  sentence   C no word character yet, uncited | D has a word character, uncited | S cited
  position   0 normal | T directly behind a run of . ! ? | TB that run plus blanks | G directly behind citations that
             followed T / TB | GB G plus blanks
  flag       an ASCII letter or _ has been seen outside a citation: only then may the answer stop (the validator wants
             at least one sentence, and a digits-only line start such as "24." is a list marker to it, not a word)
  reading    nothing | a citation (a node of the trie of the pack's ids, and the state to return to) | a prefix of a
             forbidden UTF-8 sequence | a prefix of INSUFFICIENT_EVIDENCE from the very start
`[` always opens a citation `[Q-<digits>]` / `[A-<digits>]` of the pack.  Word bytes are ASCII letters, digits, _ and
every byte >= 0x80 (a non-ASCII character may be a word character, so it asks for a citation; it may also be none, so
it does not set the flag).  A newline or a stop in D is refused: lines are sentences.  The position rules mirror the
validator's sentence cut `[.!?]+(?:[ \\t]*\\[id\\])*(?=\\s|$)`: see _step.  C0 controls other than \\n and \\t, 0x7F and
every non-ASCII code point str.isspace() knows are refused everywhere (splitlines and \\s act on them).
"""
from __future__ import annotations

import re
from collections import deque
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

DEAD = 0xFFFF
MAX_STATES = 4096
MAX_CLASSES = 64
KIND_ORDINARY, KIND_STOP, KIND_NEVER = 0, 1, 2
INSUFFICIENT = b"INSUFFICIENT_EVIDENCE"    # the reply that stands for "the evidence does not answer"; answer.py takes it from here


# ---- the automaton ---------------------------------------------------------------------------------------------------
@dataclass
class ByteDfa:
    class_of: np.ndarray      # uint8[256]
    trans: np.ndarray         # uint16[n_states, n_classes]
    accept: np.ndarray        # uint8[n_states]
    start: int = 0
    evidence_ids: Tuple[str, ...] = ()    # what citation_grammar built it from (diagnostics)
    _device: Dict[str, tuple] = field(default_factory=dict, repr=False, compare=False)

    def __post_init__(self) -> None:
        self.class_of = np.array(self.class_of, dtype=np.uint8, order="C")   # own, writable, row-major: they become tensors
        self.trans = np.array(self.trans, dtype=np.uint16, order="C")
        self.accept = np.array(self.accept, dtype=np.uint8, order="C")
        if self.class_of.shape != (256,) or self.trans.ndim != 2 or self.accept.shape != (self.trans.shape[0],):
            raise ValueError("ByteDfa: class_of must be [256], trans [n_states, n_classes] and accept [n_states]")
        if not 1 <= self.n_states <= MAX_STATES:
            raise ValueError(f"ByteDfa: {self.n_states} states, the cap is {MAX_STATES}")
        if not 1 <= self.n_classes <= MAX_CLASSES:
            raise ValueError(f"ByteDfa: {self.n_classes} byte classes, the cap is {MAX_CLASSES}")
        if int(self.class_of.max()) >= self.n_classes:
            raise ValueError("ByteDfa: class_of names a class beyond trans")
        if not 0 <= int(self.start) < self.n_states:
            raise ValueError("ByteDfa: start is not a state")

    @property
    def n_states(self) -> int:
        return int(self.trans.shape[0])

    @property
    def n_classes(self) -> int:
        return int(self.trans.shape[1])

    def to(self, device):
        """(class_of uint8, trans int16 -- the uint16 bits --, accept uint8) as tensors on `device`."""
        import torch
        key = str(device)
        if key not in self._device:
            self._device[key] = (torch.from_numpy(self.class_of).to(device),
                                 torch.from_numpy(self.trans.view(np.int16)).to(device),
                                 torch.from_numpy(self.accept).to(device))
        return self._device[key]


def walk(dfa: ByteDfa, state: Optional[int], data: bytes) -> Optional[int]:
    """The state behind `data` read from `state`; None once the walk is dead."""
    if state is None or not 0 <= state < dfa.n_states:
        return None
    for b in data:
        nxt = int(dfa.trans[state, dfa.class_of[b]])
        if nxt >= dfa.n_states:
            return None
        state = nxt
    return state


def accepts(dfa: ByteDfa, data: bytes) -> bool:
    end = walk(dfa, dfa.start, data)
    return end is not None and bool(dfa.accept[end])


# ---- the citation grammar --------------------------------------------------------------------------------------------
_ID = re.compile(r"(Q|A)-(0|[1-9][0-9]*)")
# byte categories
_NL, _BL, _TERM, _LB, _LETTER, _DIGIT, _HI, _OTHER, _FORBIDDEN = range(9)
# the UTF-8 encodings of the non-ASCII code points with str.isspace(): U+0085, U+00A0, U+1680, U+2000-U+200A, U+2028,
# U+2029, U+202F, U+205F, U+3000
_SPACES = [b"\xc2\x85", b"\xc2\xa0", b"\xe1\x9a\x80", b"\xe2\x80\xa8", b"\xe2\x80\xa9", b"\xe2\x80\xaf", b"\xe2\x81\x9f",
           b"\xe3\x80\x80"] + [bytes([0xE2, 0x80, 0x80 + i]) for i in range(11)]
_SPACE_PREFIXES = sorted({s[:k] for s in _SPACES for k in range(1, len(s))})   # a state holds index + 1: 0 is "none"


def _category(b: int) -> int:
    if b == 0x0A:
        return _NL
    if b in (0x20, 0x09):
        return _BL
    if b < 0x20 or b == 0x7F:
        return _FORBIDDEN
    if b >= 0x80:
        return _HI
    ch = chr(b)
    if ch in ".!?":
        return _TERM
    if ch == "[":
        return _LB
    if ch.isalpha() or ch == "_":
        return _LETTER
    if ch.isdigit():
        return _DIGIT
    return _OTHER


def _space_step(prefix: int, b: int) -> Optional[int]:
    """Substring matching of the forbidden sequences: `prefix` indexes _SPACE_PREFIXES + 1 (0: none).  Returns the new
    index, or None when b completes a forbidden sequence.  A byte that does not go on may itself start a prefix."""
    held = _SPACE_PREFIXES[prefix - 1] if prefix else b""
    for cand in (held + bytes([b]), bytes([b])):
        if cand in _SPACES:
            return None
        if cand in _SPACE_PREFIXES:
            return _SPACE_PREFIXES.index(cand) + 1
    return 0


def _step(sent: str, pos: str, cat: int):
    """(sentence, position) behind a byte of category cat that is not inside a citation: a pair, None (refused), or
    ("cite", sentence, position): a citation opens and returns to that pair behind its `]`."""
    word = cat in (_LETTER, _DIGIT, _HI)
    if cat == _FORBIDDEN:
        return None
    if pos == "TB" and sent != "D" and cat not in (_BL, _LB):
        sent, pos = "C", "0"       # the sentence has been cut behind the blanks: a new one begins
    if pos == "GB" and cat not in (_BL, _LB):
        pos = "0"                  # (C, GB): the citations bound backwards, what follows is a new sentence
    if pos == "0":
        if cat == _LB:
            return ("cite", "S", "0")
        if cat == _NL:
            return None if sent == "D" else ("C", "0")
        if cat == _TERM:
            return (sent, "T")
        if word:
            return ("D" if sent == "C" else sent, "0")
        return (sent, "0")
    if pos == "T":
        if cat == _TERM:
            return (sent, "T")
        if cat == _BL:
            return (sent, "TB")
        if cat == _LB:
            return ("cite", sent, "G")
        if cat == _NL:
            return None if sent == "D" else ("C", "0")
        if sent == "D":            # no whitespace follows, so the sentence goes on ("v1.2.3", 'e.g."')
            return None if cat == _HI else ("D", "0")
        if word:
            return ("D" if sent == "C" else "S", "0")
        return (sent, "0")
    if pos == "TB":                # D, or a blank / [ behind C and S
        if cat == _BL:
            return (sent, "TB")
        if cat == _LB:
            return ("cite", sent, "G")
        return None                # "Foo. bar": the validator has cut an uncited sentence
    if pos == "G":
        if cat == _LB:
            return ("cite", sent, "G")
        if cat == _BL:
            return ("C", "GB")     # whitespace follows: the group belongs to the sentence before it
        if cat == _NL:
            return ("C", "0")
        if sent == "D":
            return None            # "Foo. [Q-1]x": the validator cuts behind "Foo." and leaves it uncited
        return ("S", "T") if cat == _TERM else ("S", "0")
    if pos == "GB":                # blank or [
        return ("C", "GB") if cat == _BL else ("cite", "C", "G")
    raise AssertionError(pos)


def _build_trie(ids: Sequence[str]):
    """children[node] = {byte: node}, terminal = nodes behind a whole id."""
    children: List[Dict[int, int]] = [{}]
    terminal = set()
    for text in ids:
        node = 0
        for b in text.encode("ascii"):
            if b not in children[node]:
                children.append({})
                children[node][b] = len(children) - 1
            node = children[node][b]
        terminal.add(node)
    return children, terminal


def citation_grammar(evidence_ids: Iterable[str], allow_insufficient: bool = True) -> ByteDfa:
    """The automaton of the module docstring for a pack's evidence ids ("Q-123", "A-45").  ValueError: no id, an id of
    another form, or more states / byte classes than the caps allow."""
    ids = sorted({str(e) for e in evidence_ids})
    if not ids:
        raise ValueError("citation_grammar: no evidence id")
    for e in ids:
        if not _ID.fullmatch(e):
            raise ValueError(f"citation_grammar: {e!r} is not an evidence id of the form Q-<n> / A-<n>")
    children, terminal = _build_trie(ids)
    close = ord("]")

    # a state: (sentence, position, flag, mode, arg); mode "n" nothing, "c" citation (arg: trie node; the triple is the
    # state to return to), "u" forbidden-UTF-8 prefix (arg: its index), "i" arg bytes of INSUFFICIENT from the start
    def delta(state, b: int):
        sent, pos, flag, mode, arg = state
        if mode == "c":
            nxt = children[arg].get(b)
            if nxt is not None:
                return (sent, pos, flag, "c", nxt)
            return (sent, pos, flag, "n", 0) if b == close and arg in terminal else None
        if mode == "i" and arg < len(INSUFFICIENT) and b == INSUFFICIENT[arg]:
            return ("D", "0", 1, "i", arg + 1)
        cat = _category(b)
        prefix = 0
        if cat == _HI:
            prefix = _space_step(arg if mode == "u" else 0, b)
            if prefix is None:
                return None
        to = _step(sent, pos, cat)
        if to is None:
            return None
        if to[0] == "cite":
            return (to[1], to[2], flag, "c", 0)
        return (to[0], to[1], 1 if cat == _LETTER else flag, "u" if prefix else "n", prefix)

    def accepting(state) -> bool:
        sent, pos, flag, mode, arg = state
        if mode == "i":
            return arg == len(INSUFFICIENT)
        return mode == "n" and bool(flag) and (sent != "D" or pos == "G")

    start = ("C", "0", 0, "i" if allow_insufficient else "n", 0)
    index = {start: 0}
    order = [start]
    rows: List[List[int]] = []
    queue = deque([start])
    while queue:
        state = queue.popleft()
        row = []
        for b in range(256):
            nxt = delta(state, b)
            if nxt is None:
                row.append(DEAD)
                continue
            if nxt not in index:
                if len(order) >= MAX_STATES:
                    raise ValueError(f"citation_grammar: {len(ids)} ids need more than {MAX_STATES} states")
                index[nxt] = len(order)
                order.append(nxt)
                queue.append(nxt)
            row.append(index[nxt])
        rows.append(row)
    full = np.asarray(rows, dtype=np.uint16)                     # [n_states, 256], rows in discovery order
    columns, class_of = np.unique(full, axis=1, return_inverse=True)   # bytes with the same column share a class
    if columns.shape[1] > MAX_CLASSES:
        raise ValueError(f"citation_grammar: {columns.shape[1]} byte classes, the cap is {MAX_CLASSES}")
    accept = np.asarray([accepting(s) for s in order], dtype=np.uint8)
    return ByteDfa(class_of=np.asarray(class_of).reshape(256), trans=columns, accept=accept, start=0,
                   evidence_ids=tuple(ids))


# ---- the vocabulary ---------------------------------------------------------------------------------------------------
def _gpt2_unicode_to_byte() -> Dict[str, int]:
    """The inverse of the byte -> printable character alphabet of byte-level BPE (GPT-2's bytes_to_unicode)."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    chars = list(keep)
    extra = 0
    for b in range(256):
        if b not in keep:
            keep.append(b)
            chars.append(256 + extra)
            extra += 1
    return {chr(c): b for b, c in zip(keep, chars)}


class TokenTable:
    """offsets int32[V + 1] / bytes uint8: the raw bytes of every token id; kind uint8[V]."""

    def __init__(self, offsets: np.ndarray, data: np.ndarray, kind: np.ndarray) -> None:
        self.offsets = np.array(offsets, dtype=np.int32, order="C")      # own, writable copies: they become tensors
        self.bytes = np.array(data, dtype=np.uint8, order="C")
        self.kind = np.array(kind, dtype=np.uint8, order="C")
        if self.offsets.ndim != 1 or self.offsets.size != self.kind.size + 1 or self.offsets[0] != 0 \
                or np.any(np.diff(self.offsets) < 0) or int(self.offsets[-1]) > self.bytes.size or self.bytes.size == 0:
            raise ValueError("TokenTable: offsets must rise from 0 to at most len(bytes), one more than kind")
        self._device: Dict[str, tuple] = {}

    @property
    def vocab(self) -> int:
        return int(self.kind.size)

    def token_bytes(self, token: int) -> bytes:
        return self.bytes[self.offsets[token]:self.offsets[token + 1]].tobytes()

    @classmethod
    def from_bytes(cls, tokens: Sequence[Optional[bytes]], stop_ids: Iterable[int] = (),
                   never_ids: Iterable[int] = ()) -> "TokenTable":
        """tokens[id] = the id's raw bytes (None or b"": none).  stop_ids get kind 1; never_ids and ordinary ids with
        no bytes get kind 2."""
        stop, never = {int(s) for s in stop_ids}, {int(s) for s in never_ids}
        blobs = [bytes(t or b"") for t in tokens]
        kind = np.zeros(len(blobs), dtype=np.uint8)
        for i, blob in enumerate(blobs):
            kind[i] = KIND_STOP if i in stop else KIND_NEVER if (i in never or not blob) else KIND_ORDINARY
        offsets = np.zeros(len(blobs) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in blobs], out=offsets[1:])
        if offsets[-1] > 0x7FFFFFFF:
            raise ValueError("TokenTable: the vocabulary's bytes do not fit 32-bit offsets")
        data = np.frombuffer(b"".join(blobs) or b"\0", dtype=np.uint8)   # never empty: the kernel takes no NULL table
        return cls(offsets.astype(np.int32), data, kind)

    @classmethod
    def from_tokenizer(cls, tokenizer, stop_ids: Iterable[int] = (), vocab_size: Optional[int] = None) -> "TokenTable":
        """The table of a byte-level BPE tokenizer (Qwen's, GPT-2's): every id's token string mapped back through the
        byte alphabet.  Added / special tokens, ids the tokenizer does not know (a model's padded vocabulary:
        vocab_size) and strings outside the alphabet are never allowed, unless they are stop ids."""
        n = max(int(vocab_size or 0), len(tokenizer))
        to_byte = _gpt2_unicode_to_byte()
        special = {int(i) for i in getattr(tokenizer, "all_special_ids", [])}
        special |= {int(i) for i in (tokenizer.get_added_vocab() or {}).values()}
        strings = tokenizer.convert_ids_to_tokens(list(range(len(tokenizer))))
        tokens: List[Optional[bytes]] = [None] * n
        for i, text in enumerate(strings):
            if i in special or not text:
                continue
            try:
                tokens[i] = bytes(to_byte[ch] for ch in text)
            except KeyError:
                pass
        return cls.from_bytes(tokens, stop_ids, never_ids=special)

    def to(self, device):
        """(offsets int32, bytes uint8, kind uint8) as tensors on `device`; built once per device."""
        import torch
        key = str(device)
        if key not in self._device:
            self._device[key] = (torch.from_numpy(self.offsets).to(device), torch.from_numpy(self.bytes).to(device),
                                 torch.from_numpy(self.kind).to(device))
        return self._device[key]


@dataclass
class TokenGrammar:
    """What a generator needs to decode under an automaton.  table None: the generator uses its own cached table."""
    dfa: ByteDfa
    table: Optional[TokenTable] = None


# ---- the host rule ----------------------------------------------------------------------------------------------------
def _walk_all(dfa: ByteDfa, table: TokenTable, state: int) -> np.ndarray:
    """int32[V]: the end state of every token's bytes read from `state`, -1 where the walk dies or there are no bytes."""
    lens = np.diff(table.offsets).astype(np.int64)
    cur = np.where(lens > 0, int(state), -1).astype(np.int64)
    if not 0 <= int(state) < dfa.n_states:
        cur[:] = -1
    trans = dfa.trans.astype(np.int64)
    for k in range(int(lens.max()) if lens.size else 0):
        idx = np.nonzero((lens > k) & (cur >= 0))[0]
        if idx.size == 0:
            break
        nxt = trans[cur[idx], dfa.class_of[table.bytes[table.offsets[idx] + k]]]
        cur[idx] = np.where(nxt < dfa.n_states, nxt, -1)
    return cur.astype(np.int32)


def allowed_tokens_host(dfa: ByteDfa, table: TokenTable, state: int) -> np.ndarray:
    """bool[V]: a stop token in an accepting state; an ordinary token with bytes whose walk from `state` stays alive."""
    ok_state = 0 <= int(state) < dfa.n_states
    ends = _walk_all(dfa, table, state)
    stop_ok = ok_state and bool(dfa.accept[int(state)])
    return ((table.kind == KIND_ORDINARY) & (ends >= 0)) | ((table.kind == KIND_STOP) & stop_ok)


def next_state_host(dfa: ByteDfa, table: TokenTable, state: int, token: int) -> int:
    """The state behind an allowed token: unchanged for a stop token (and for -1, nothing chosen)."""
    if token < 0 or table.kind[token] == KIND_STOP:
        return int(state)
    end = walk(dfa, int(state), table.token_bytes(token))
    if end is None or table.kind[token] != KIND_ORDINARY:
        raise ValueError(f"token {token} is not allowed in state {state}")
    return end


def argmax_host(logits: np.ndarray, allowed: np.ndarray) -> int:
    """The lowest id among the maxima of logits over allowed, NaNs left out; -1 when nothing is left."""
    idx = np.nonzero(allowed & ~np.isnan(logits))[0]
    return int(idx[np.argmax(logits[idx])]) if idx.size else -1
