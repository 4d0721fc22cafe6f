"""Rule sets whose states differ, for the token-rule kernels (csrc/step_rules.h, csrc/beam_rules.h), numpy only.  Holds no tests.

tests/test_gpu_rules.py's counter_rules and close_ref.closing_counter_rules stack ONE row twice, move the depth by -1 / 0 / +1 and keep
dist[s][d] = d + 1 in every state: a kernel that read the wrong state's row, sign-extended delta wrongly, forgot a clamp or indexed the
distance table by the wrong state picks the same tokens under them.  Every member here has rows that differ by state (the class of a token
is (id + 2 * s) % 7), deltas of -2 and below, a token that clamps at depth 0, a distance table that depends on the state, and -- `wide` --
the full 8 x 256 table.  Each builder takes (V, eos, banned=()) and returns a TokenRules that passes validate(V); tests/test_rule_zoo_cpu.py
pins the tables and the structural facts the GPU tests rely on."""
import json
import os
from typing import NamedTuple, Tuple

import numpy as np

from texocr_amd import rules as R

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(V, eos, banned, S, depth_max, deltas, needs, active, nxt, eos_states):
    """class c = (id + 2 * s) % 7 of token id in state s takes (deltas[c], needs[c]) where active(c, s), and is neutral where not;
    next = nxt(ids, s, lowering: the entry lowers the depth).  eos: ONLY_AT_ZERO in eos_states, BAN elsewhere; `banned`: BAN."""
    ids = np.arange(V)
    table = np.zeros((S, V), dtype=np.int32)
    deltas, needs = np.asarray(deltas, dtype=np.int64), np.asarray(needs, dtype=np.int64)
    for s in range(S):
        c = (ids + 2 * s) % 7
        on = np.asarray([active(int(k), s) for k in range(7)], dtype=bool)[c]
        delta, need = np.where(on, deltas[c], 0), np.where(on, needs[c], 0)
        flags = np.zeros(V, dtype=np.int64)
        flags[np.asarray(sorted(banned), dtype=np.int64)] = R.BAN
        delta[eos], need[eos], flags[eos] = 0, 0, R.ONLY_AT_ZERO if s in eos_states else R.BAN
        nx = nxt(ids, s, delta < 0)
        nx[eos] = s                                               # (the eos leaves the state where it was)
        table[s] = R.pack(need=need, delta=delta, next=nx, flags=flags)
    return R.TokenRules(table, depth_max).validate(V)


# class:        0      1      2         3         4            5        6
SKEW_DELTAS = (+1,    +2,    -1,       -3,       -2,          0,       0)      # open, open two, close, close three, drop (clamps), neutral
SKEW_NEEDS = (0,      0,     1,        3,        0,           0,       0)


def skew(V, eos, banned=(), S=3, depth_max=12, eos_states=(0,), trap=None):
    """S states.  Class (id + 2 * s) % 7: open +1, open +2, close -1 (need 1), close -3 (need 3), drop -2 (need 0: clamps at depth 0),
    two neutral classes.  The -3 class lowers in state 0 only and the drop in states 0 and 1 (neutral elsewhere); a lowering token keeps
    the state, every other has next = (id + s) % S; eos is ONLY_AT_ZERO in eos_states and banned in the other states.  So dist depends on
    the state at every depth -- a row in state 2 has to walk to state 0 or close one by one -- and dist_max is 6 at depth_max = 12.
    trap = s: state s is absorbing (next = s on its whole row) and its eos is banned."""
    def active(c, s):
        return c not in (3, 4) or s == 0 or (c == 4 and s == 1)

    def nxt(ids, s, lowering):
        if trap is not None and s == trap:
            return np.full(ids.shape, s)
        return np.where(lowering, s, (ids + s) % S)
    return _build(V, eos, banned, S, depth_max, SKEW_DELTAS, SKEW_NEEDS, active, nxt, tuple(e for e in eos_states if e != trap))


def trap(V, eos, banned=(), S=3, depth_max=12):
    """skew with state 2 absorbing and without an eos: close_dist has any_inf, state 2 infinite at every depth; under the plain rule the
    tokens into state 2 are ordinary allowed tokens"""
    return skew(V, eos, banned, S, depth_max, trap=2)


def wide(V, eos, banned=(), S=8, depth_max=255):
    """deltas +1, +half, -1, -(half + 1) (need half + 1), a drop of -(2 * depth_max // 5) with need 0 (clamps), -(depth_max // 6) with its
    need, neutral -- at depth_max = 255: +1, +127, -1, -128, -102, -42.  The -(half + 1) class lowers in state 4 % S only, the
    drop in state 0 only; next = (m * id + s) % S with m = 5 (3 where 5 divides S); eos ONLY_AT_ZERO in states 0 and 5 % S.
    S = 8: the full 2048-node table; S = 5: 1280 nodes, 160 whole 16-byte pieces; S = 3, depth_max = 100: 303 nodes, a partial last piece."""
    half = depth_max // 2
    big, drop, mid = min(half + 1, 128), (2 * depth_max) // 5, max(depth_max // 6, 2)
    deltas = (+1, +half, -1, -big, -drop, -mid, 0)
    needs = (0, 0, 1, big, 0, mid, 0)
    m = 3 if S % 5 == 0 else 5
    return _build(V, eos, banned, S, depth_max, deltas, needs, lambda c, s: (c != 3 or s == 4 % S) and (c != 4 or s == 0),
                  lambda ids, s, lowering: (m * ids + s) % S, (0, 5 % S))


def tok1k():
    from texocr_amd.tokenizer import RegExTokenizer
    v = json.load(open(os.path.join(HERE, "golden", "tokenizer_vocab_1k.json")))
    return RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"])


def brace1k(V=1000, eos=997, banned=(998, 999), depth_max=64):
    """rules.brace_rules over tests/golden/tokenizer_vocab_1k.json: the one two-state rule set of the package whose rows differ"""
    return R.brace_rules(tok1k(), depth_max=depth_max, ban=list(banned), eos=eos, vocab=V).validate(V)


def by_delta(rules, delta, state=0, lo=None):
    """the ids whose entry in `state` is allowed somewhere and has this delta (lo given: lo <= delta' <= delta), eos-like entries apart"""
    need, dl, nxt, flags = R.unpack(rules.table[state])
    hit = (dl == delta) if lo is None else ((dl >= lo) & (dl <= delta))
    return np.nonzero(hit & (flags == 0))[0].tolist()


class Events(NamedTuple):
    states: Tuple[int, ...]   # the states the row stood in: the start state and the one behind every token
    deep_close: bool          # a token with delta <= -2 was committed
    clamp_zero: bool          # a committed token took the depth below 0 (clamped)
    clamp_max: bool           # a committed token took the depth above depth_max (clamped: only a forced token can)
    max_need: int             # the largest need among the committed tokens
    max_depth: int            # the largest depth the row stood at


def events(rules, tokens, state0=None):
    """tokens (B, n) committed from state0 (B, 2) (default: the start state) -> one Events per row, by the host automaton"""
    tokens = np.asarray(tokens, dtype=np.int64)
    tokens = tokens[None] if tokens.ndim == 1 else tokens
    out = []
    for b, row in enumerate(tokens):
        st = rules.start(1)[0] if state0 is None else np.asarray(state0, dtype=np.int32).reshape(-1, 2)[b]
        s, d = int(st[0]), int(st[1])
        seen, deep, c0, cm, mneed, mdepth = [s], False, False, False, 0, d
        for t in row.tolist():
            need, delta, nxt, _ = (int(x) for x in R.unpack(rules.table[s, t]))
            deep |= delta <= -2
            c0 |= d + delta < 0
            cm |= d + delta > rules.depth_max
            mneed = max(mneed, need)
            s, d = nxt, min(max(d + delta, 0), rules.depth_max)
            seen.append(s)
            mdepth = max(mdepth, d)
        out.append(Events(tuple(seen), deep, c0, cm, mneed, mdepth))
    return out
