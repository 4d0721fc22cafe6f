"""The repeat guard (include/texocr.h: txo_set_repeat_guard) restated for the tests, by brute force and independently of
texocr_amd/guard.py.  Holds no tests.

No running counters: for every period p the candidate sequence history + [x] is built, its last (R + 1) * p tokens are cut into R + 1
windows of p tokens, and the windows are compared as blocks.  x is banned iff some p in 1 .. P makes all R + 1 windows equal."""
import numpy as np

MASKED = np.float32(-3.4e38)


def ends_in_copies(seq, p, copies):
    """does seq end in `copies` consecutive equal blocks of p tokens?"""
    seq = list(seq)
    if len(seq) < copies * p:
        return False
    tail = seq[len(seq) - copies * p:]
    windows = [tuple(tail[k * p:(k + 1) * p]) for k in range(copies)]
    return all(w == windows[0] for w in windows)


def banned(history, P, R, eos=None, vocab=None):
    """every token x (of the history's own alphabet, or of range(vocab)) whose commit would end the row in R + 1 copies of a block of p <= P"""
    history = [int(t) for t in history]
    cands = set(history) if vocab is None else range(vocab)
    return {x for x in cands if x != eos and any(ends_in_copies(history + [x], p, R + 1) for p in range(1, P + 1))}


def violations(row, P, R, eos=None):
    """positions of a row whose token was banned by the tokens before it"""
    row = [int(t) for t in row]
    return [i for i in range(len(row)) if row[i] in banned(row[:i], P, R, eos)]


def hits(row, P, R, eos=None):
    """positions of a row at which the ban set was non-empty"""
    row = [int(t) for t in row]
    return [i for i in range(len(row)) if banned(row[:i], P, R, eos)]


def mask(logits_row, history, P, R, eos=None, allowed=None):
    """the row the selection sees: MASKED where banned or (allowed: a bool (V,) from the token rules) disallowed; if nothing is both allowed
    and unbanned the ban is dropped -> (masked row float32, the ban set, yielded)"""
    row = np.asarray(logits_row, dtype=np.float32)
    ok = np.ones(row.shape[0], dtype=bool) if allowed is None else np.asarray(allowed, dtype=bool)
    ban = banned(history, P, R, eos)
    free = ok.copy()
    free[sorted(ban)] = False
    yielded = not free.any()
    keep = ok if yielded else free
    return np.where(keep, row, MASKED), ban, yielded
