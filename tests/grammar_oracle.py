"""Helpers of the grammar tests (test_grammar_host.py, test_grammar_gpu.py): graph searches over a ByteDfa, seeded random
walks finished by a shortest path to acceptance, and the synthetic vocabulary the kernel is checked on."""
from __future__ import annotations

from collections import deque
from typing import Dict, List, Optional, Tuple

import numpy as np

from cadence_rag_amd.grammar import ByteDfa, TokenTable

IDS = ["Q-12", "Q-123", "A-45", "Q-7"]
# letters, digits, _ . ! ? , " ) ] [ - Q A, space, tab, newline and the two bytes of "é"
ALPHABET = sorted(set(b"abcxyzINSUFTEVDQA0123456789_.!?,\")][- \t\n" + "é".encode()))


def byte_table(dfa: ByteDfa) -> np.ndarray:
    """int32[n_states, 256]: the next state per byte, -1 dead."""
    full = dfa.trans[:, dfa.class_of].astype(np.int32)
    full[full >= dfa.n_states] = -1
    return full


def reachable(dfa: ByteDfa) -> List[int]:
    """Every state a byte string can reach from the start, in breadth-first order."""
    table = byte_table(dfa)
    seen, order, queue = {dfa.start}, [dfa.start], deque([dfa.start])
    while queue:
        for nxt in np.unique(table[queue.popleft()]):
            if nxt >= 0 and int(nxt) not in seen:
                seen.add(int(nxt))
                order.append(int(nxt))
                queue.append(int(nxt))
    return order


def completions(dfa: ByteDfa, alphabet=range(256)) -> Dict[int, bytes]:
    """state -> a shortest byte string over `alphabet` that leads it to an accepting state (states that reach none are
    missing).  Breadth-first over the reversed graph from the accepting states."""
    table = byte_table(dfa)
    back: Dict[int, List[Tuple[int, int]]] = {}
    for s in range(dfa.n_states):
        for b in alphabet:
            t = int(table[s, b])
            if t >= 0:
                back.setdefault(t, []).append((s, b))
    out: Dict[int, bytes] = {int(s): b"" for s in np.nonzero(dfa.accept)[0]}
    queue = deque(out)
    while queue:
        t = queue.popleft()
        for s, b in back.get(t, ()):
            if s not in out:
                out[s] = bytes([b]) + out[t]
                queue.append(s)
    return out


def alive_bytes(dfa: ByteDfa, alphabet=ALPHABET) -> List[List[Tuple[int, int]]]:
    """Per state the (byte, next state) pairs of the alphabet bytes that are alive in it."""
    table = byte_table(dfa)
    return [[(b, int(table[s, b])) for b in alphabet if table[s, b] >= 0] for s in range(dfa.n_states)]


def random_walk(dfa: ByteDfa, alive: List[List[Tuple[int, int]]], rng, steps: int) -> Tuple[bytes, int]:
    """`steps` bytes drawn uniformly (rng: random.Random) among the bytes alive in the current state: (bytes, end state)."""
    state, out = dfa.start, bytearray()
    for _ in range(steps):
        if not alive[state]:
            break
        b, state = alive[state][rng.randrange(len(alive[state]))]
        out.append(b)
    return bytes(out), state


# ---- the synthetic vocabulary of the kernel tests ------------------------------------------------------------------
PLANTED = [b"[Q-12]", b" [Q", b"-12", b"].", b"] ", b".[", b"3]\n", b"Foo", b" bar", b"[A-45]", b"[Q-7]", b"Q-1", b"23]",
           b". ", b".\n", b"INSUFFICIENT", b"_EVIDENCE"]
VOCAB = 3001          # no multiple of 32, 64 or 1024


def synthetic_vocab(seed: int = 11) -> Tuple[TokenTable, Dict[str, List[int]]]:
    """3001 tokens: the 256 single bytes, seeded random strings of 2-12 bytes over the walk alphabet, the planted tokens
    that cross every boundary of a citation, one 40-byte token, three ids with no bytes, two kind-2 tokens with bytes,
    two stop ids -- shuffled, so that no kind sits at one end of the id range."""
    rng = np.random.default_rng(seed)
    tokens: List[Optional[bytes]] = [bytes([b]) for b in range(256)] + list(PLANTED)
    tokens.append(b"the answer is in the summary of the call")          # 40 bytes
    assert len(tokens[-1]) == 40
    special = {"empty": [], "never": [], "stop": []}
    tokens += [b"", None, b""]                                               # no bytes
    tokens += [b"<never-1>", b"ok"]                                          # kind 2 although "ok" would walk
    tokens += [b"<stop-1>", b"<stop-2>"]
    alpha = np.asarray(ALPHABET, dtype=np.uint8)
    while len(tokens) < VOCAB:
        tokens.append(alpha[rng.integers(0, alpha.size, int(rng.integers(2, 13)))].tobytes())
    first_special = 256 + len(PLANTED) + 1
    perm = rng.permutation(VOCAB)
    shuffled: List[Optional[bytes]] = [None] * VOCAB
    for old, new in enumerate(perm):
        shuffled[int(new)] = tokens[old]
    for name, olds in (("empty", range(first_special, first_special + 3)),
                       ("never", range(first_special + 3, first_special + 5)),
                       ("stop", range(first_special + 5, first_special + 7))):
        special[name] = sorted(int(perm[o]) for o in olds)
    table = TokenTable.from_bytes(shuffled, stop_ids=special["stop"], never_ids=special["never"])
    return table, special
