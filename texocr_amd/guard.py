"""The repeat guard (include/texocr.h: txo_set_repeat_guard; csrc/step_guard.h) in numpy: which tokens a row may not pick next, and where
a finished row was (or would have been) held back.  Callers use `hits` to flag looped rows of an unguarded decode.

A guard is two integers, max_period P and max_repeats R, both in 1 .. 16.  With a row's history h[0 .. n-1] (every token committed behind
the start token) and a period p in 1 .. P, p <= n: m_p = the number of trailing positions i with i - p >= 0 and h[i] == h[i - p], counted
back from n - 1 to the first mismatch; token h[n - p] is banned iff m_p >= R * p - 1.  The eos token is never banned."""
from __future__ import annotations

import numpy as np

GUARD_MAX = 16


def check(repeat_guard, vocab=None):
    """(P, R) as the engine accepts it, or ValueError with the engine's text -> (P, R) as ints; None passes through"""
    if repeat_guard is None:
        return None
    try:
        P, R = repeat_guard
        if isinstance(P, bool) or isinstance(R, bool) or int(P) != P or int(R) != R:
            raise TypeError
        P, R = int(P), int(R)
    except (TypeError, ValueError):
        raise ValueError("repeat guard: repeat_guard must be a pair of integers (max_period, max_repeats)") from None
    if not 1 <= P <= GUARD_MAX:
        raise ValueError(f"repeat guard: max_period is {P}; it must be in [1, {GUARD_MAX}] (0, 0 switches the guard off)")
    if not 1 <= R <= GUARD_MAX:
        raise ValueError(f"repeat guard: max_repeats is {R}; it must be in [1, {GUARD_MAX}] (0, 0 switches the guard off)")
    if vocab is not None and vocab <= P + 1:
        raise ValueError(f"repeat guard: the vocabulary has {vocab} entries; it needs more than max_period + 1 = {P + 1} "
                         "(the guard may ban max_period tokens at a pick)")
    return P, R


def banned(history, P, R, eos=None) -> set:
    """the tokens the guard (P, R) bans at the pick behind `history` (a sequence of token ids)"""
    h = np.asarray(history, dtype=np.int64).reshape(-1)
    n = h.shape[0]
    out = set()
    for p in range(1, min(P, n) + 1):
        m = 0
        while m < R * p - 1 and n - 1 - m - p >= 0 and h[n - 1 - m] == h[n - 1 - m - p]:
            m += 1
        if m >= R * p - 1:
            out.add(int(h[n - p]))
    out.discard(None if eos is None else int(eos))
    return out


def hits(tokens, P, R, eos=None) -> list:
    """tokens (B, n) or (n,): per row, the positions at which the ban set was non-empty (a guarded decode had fewer tokens to choose from
    there; in an unguarded one, a position whose token is in the set is where a loop began)"""
    t = np.asarray(tokens, dtype=np.int64)
    rows = t[None, :] if t.ndim == 1 else t
    return [[i for i in range(row.shape[0]) if banned(row[:i], P, R, eos)] for row in rows]


def violations(tokens, P, R, eos=None) -> list:
    """per row, the positions whose token the guard (P, R) would have banned: where the row completed an (R + 1)-th copy of a block"""
    t = np.asarray(tokens, dtype=np.int64)
    rows = t[None, :] if t.ndim == 1 else t
    return [[i for i in range(row.shape[0]) if int(row[i]) in banned(row[:i], P, R, eos)] for row in rows]
