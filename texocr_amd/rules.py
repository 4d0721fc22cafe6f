"""Token rules of a constrained decode (include/texocr.h: txo_set_token_rules; csrc/step_rules.h), numpy only.

A rule set is a table ``rules[S][V]`` of packed int32 -- S automaton states (1 .. 8), V the vocabulary -- and a scalar ``depth_max``
(1 .. 255).  An entry packs ``need`` (bits 0-7, unsigned), ``delta`` (bits 8-15, signed), ``next`` (bits 16-23) and the flags BAN (bit 24)
and ONLY_AT_ZERO (bit 25).  Every row of a batch carries a state ``(s, depth)``, ``(0, 0)`` at the start.  In ``(s, depth)`` token v with
``r = rules[s][v]`` is allowed iff

    not BAN   and   depth >= need   and   depth + delta <= depth_max   and   (not ONLY_AT_ZERO or depth == 0)

and committing a token -- picked or forced by a prefix -- moves the row to ``(next, clamp(depth + delta, 0, depth_max))``.  A disallowed
logit counts as ``MASKED`` (-3.4e38f) in the selection.  ``TokenRules.step`` is this rule on the host: the one restatement every layer and
every test shares."""
from __future__ import annotations

from typing import Iterable, Optional, Sequence, Tuple

import numpy as np

BAN, ONLY_AT_ZERO = 1, 2            # the flag bits of an entry (bits 24 and 25 of the packed word)
MAX_STATES = 8
MASKED = np.float32(-3.4e38)        # what a disallowed logit counts as
CLOSE_INF = np.int32(0x7fffffff)    # a close_dist entry without a path to eos (include/texocr.h: TXO_CLOSE_INF)


def pack(need=0, delta=0, next=0, flags=0) -> np.ndarray:
    """entries from their fields (broadcast) -> int32; need 0 .. 255, delta -128 .. 127, next 0 .. 255, flags of BAN | ONLY_AT_ZERO"""
    need, delta, next, flags = (np.asarray(x, dtype=np.int64) for x in (need, delta, next, flags))
    if ((need < 0) | (need > 255)).any() or ((delta < -128) | (delta > 127)).any() or ((next < 0) | (next > 255)).any() or ((flags < 0) | (flags > 3)).any():
        raise ValueError("token rules: need must be in [0, 255], delta in [-128, 127], next in [0, 255], flags in [0, 3]")
    return (need | ((delta & 0xff) << 8) | (next << 16) | (flags << 24)).astype(np.int32)


def unpack(entry) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """int32 entries -> (need, delta, next, flags), each an int32 array of the same shape"""
    e = np.asarray(entry, dtype=np.int32).astype(np.int64) & 0xffffffff
    delta = (e >> 8) & 0xff
    return ((e & 0xff).astype(np.int32), np.where(delta >= 128, delta - 256, delta).astype(np.int32), ((e >> 16) & 0xff).astype(np.int32),
            ((e >> 24) & 0xff).astype(np.int32))


class CloseDist(np.ndarray):
    """TokenRules.close_dist's table: int32 (S, depth_max + 1), CLOSE_INF where eos cannot be reached, with the eos id it was computed for
    (``eos``), its largest finite entry (``dist_max``, 0: none) and ``any_inf``"""
    eos: int = -1
    dist_max: int = 0
    any_inf: bool = True

    def __array_finalize__(self, obj):
        if obj is not None:
            self.eos, self.dist_max, self.any_inf = getattr(obj, "eos", -1), getattr(obj, "dist_max", 0), getattr(obj, "any_inf", True)


class TokenRules:
    """table (S, V) int32 of packed entries and depth_max.  ``validate()`` raises what the engine refuses at installation."""

    def __init__(self, table, depth_max: int):
        self.table = np.ascontiguousarray(np.asarray(table, dtype=np.int32))
        self.depth_max = int(depth_max)

    @property
    def n_states(self) -> int:
        return int(self.table.shape[0])

    @property
    def vocab(self) -> int:
        return int(self.table.shape[1])

    def validate(self, vocab: Optional[int] = None) -> "TokenRules":
        """The engine's own checks, in its order (ValueError naming the rule): S in [1, 8], depth_max in [1, 255], every next < S, every state
        with a token that is allowed at every depth (not BAN, not ONLY_AT_ZERO, need == 0, delta <= 0), V == vocab where given."""
        if self.table.ndim != 2:
            raise ValueError("token rules: the table must have the shape (S, V)")
        S, V = self.table.shape
        if not 1 <= S <= MAX_STATES:
            raise ValueError(f"token rules: S is {S}; the number of states must be in [1, {MAX_STATES}]")
        if not 1 <= self.depth_max <= 255:
            raise ValueError(f"token rules: depth_max is {self.depth_max}; it must be in [1, 255]")
        if V < 1:
            raise ValueError("token rules: V must be >= 1")
        need, delta, nxt, flags = unpack(self.table)
        for s in range(S):
            bad = np.nonzero(nxt[s] >= S)[0]
            if bad.size:
                raise ValueError(f"token rules: rules[{s}][{int(bad[0])}] has next = {int(nxt[s, bad[0]])}, not a state below S = {S}")
            if not ((flags[s] & (BAN | ONLY_AT_ZERO) == 0) & (need[s] == 0) & (delta[s] <= 0)).any():
                raise ValueError(f"token rules: state {s} has no always-allowed token (not BAN, not ONLY_AT_ZERO, need == 0, delta <= 0): "
                                 "a row could face an empty allowed set")
        if vocab is not None and V != int(vocab):
            raise ValueError(f"token rules: V is {V} but the engine's vocabulary has {int(vocab)} entries")
        return self

    def start(self, rows: int) -> np.ndarray:
        return np.zeros((int(rows), 2), dtype=np.int32)

    def allowed(self, state, remaining=None, ended=None, dist=None) -> np.ndarray:
        """state (n, 2) of (s, depth) -> (n, V) bool: the tokens every row may pick.
        remaining= (n,) or a scalar: the closing decode's rule (txo_set_rules_close) -- R, the picks every row has left in what the call
        returns, this one included; dist= the CloseDist of close_dist(eos) (needed then); ended= (n,) bool, rows that have committed an eos
        (default: none).  A row that has not ended, with D = dist[s][depth] finite, may pick v iff the rule allows it and (v == eos or
        dist[next][depth after v] <= max(R, D) - 1); an ended row and a row with D infinite keep the plain rule."""
        state = np.asarray(state, dtype=np.int32).reshape(-1, 2)
        need, delta, nxt, flags = unpack(self.table[state[:, 0]])
        depth = state[:, 1:2]
        ok = ((flags & BAN) == 0) & (depth >= need) & (depth + delta <= self.depth_max) & (((flags & ONLY_AT_ZERO) == 0) | (depth == 0))
        if remaining is None:
            if ended is not None or dist is not None:
                raise ValueError("token rules: ended= and dist= belong to remaining= (the closing decode's rule)")
            return ok
        if not isinstance(dist, CloseDist) or dist.shape != (self.n_states, self.depth_max + 1):
            raise ValueError("token rules: remaining= needs dist=, the table close_dist(eos) returned for these rules")
        n = state.shape[0]
        R = np.broadcast_to(np.asarray(remaining, dtype=np.int64).reshape(-1), (n,))
        done = np.zeros(n, dtype=bool) if ended is None else np.broadcast_to(np.asarray(ended, dtype=bool).reshape(-1), (n,))
        d64 = np.asarray(dist, dtype=np.int64)
        D = d64[state[:, 0], state[:, 1]]
        bind = ~done & (D != int(CLOSE_INF))
        lim = np.maximum(R, D) - 1
        after = d64[np.minimum(nxt, self.n_states - 1), np.clip(depth + delta, 0, self.depth_max)]
        close = after <= lim[:, None]                              # (CLOSE_INF never is: lim is finite where the row binds)
        close[:, dist.eos] = True
        return np.where(bind[:, None], ok & close, ok)

    def mask(self, state, logits, remaining=None, ended=None, dist=None) -> np.ndarray:
        """the float32 rows the selection sees: logits (n, V) with MASKED where a token is disallowed (remaining / ended / dist: as allowed)"""
        return np.where(self.allowed(state, remaining, ended, dist), np.asarray(logits, dtype=np.float32), MASKED)

    def close_dist(self, eos: int) -> CloseDist:
        """The closing decode's table (csrc/rules_close.h restated): dist[s][d] = the least number of picks, the eos included, that takes a
        row from (s, d) to a committed eos with every pick allowed and every move the rule's own; CLOSE_INF: no path."""
        S, W = self.n_states, self.depth_max + 1
        out = np.full((S, W), int(CLOSE_INF), dtype=np.int64)
        eos = int(eos)
        if 0 <= eos < self.vocab:
            depths = np.arange(W)
            edges = []                                             # per state: its distinct words' (allowed at d, node behind it at d), eos apart
            for s in range(S):
                words = np.unique(np.delete(self.table[s], eos))
                need, delta, nxt, flags = unpack(words[:, None])
                ok = ((flags & BAN) == 0) & (depths >= need) & (depths + delta <= self.depth_max) & (((flags & ONLY_AT_ZERO) == 0) | (depths == 0))
                edges.append((ok & (nxt < S), np.minimum(nxt, S - 1) + 0 * depths, np.clip(depths + delta, 0, self.depth_max)))
            out[self.allowed(np.stack([np.repeat(np.arange(S), W), np.tile(depths, S)], 1))[:, eos].reshape(S, W)] = 1
            for level in range(2, S * W + 1):
                new = np.zeros((S, W), dtype=bool)
                for s, (ok, ns, nd) in enumerate(edges):
                    new[s] = (ok & (out[ns, nd] == level - 1)).any(0) & (out[s] == int(CLOSE_INF))
                if not new.any():
                    break
                out[new] = level
        res = out.astype(np.int32).view(CloseDist)
        finite = out[out != int(CLOSE_INF)]
        res.eos, res.dist_max, res.any_inf = eos, int(finite.max()) if finite.size else 0, bool((out == int(CLOSE_INF)).any())
        return res

    def step(self, state, tokens) -> Tuple[np.ndarray, np.ndarray]:
        """state (n, 2), tokens (n,) committed in it -> (next state (n, 2) int32, allowed (n,) bool: would the rules have let the row pick it)"""
        state = np.asarray(state, dtype=np.int32).reshape(-1, 2)
        tokens = np.asarray(tokens, dtype=np.int64).reshape(-1)
        need, delta, nxt, flags = unpack(self.table[state[:, 0], tokens])
        depth = state[:, 1]
        ok = ((flags & BAN) == 0) & (depth >= need) & (depth + delta <= self.depth_max) & (((flags & ONLY_AT_ZERO) == 0) | (depth == 0))
        return np.stack([nxt, np.clip(depth + delta, 0, self.depth_max)], 1).astype(np.int32), ok

    def run(self, tokens, state=None) -> Tuple[np.ndarray, np.ndarray]:
        """a sequence (T,) through one row's automaton -> (final state (2,), allowed (T,))"""
        st = self.start(1) if state is None else np.asarray(state, dtype=np.int32).reshape(1, 2)
        ok = np.zeros(len(tokens), dtype=bool)
        for i, t in enumerate(tokens):
            st, o = self.step(st, [t])
            ok[i] = o[0]
        return st[0], ok


def ban(V: int, ids: Iterable[int]) -> TokenRules:
    """the one-state rule set that only bans `ids`"""
    flags = np.zeros(int(V), dtype=np.int64)
    flags[np.asarray(list(ids), dtype=np.int64)] = BAN
    return TokenRules(pack(flags=flags)[None, :], 1)


def token_braces(data: bytes, escaped: bool) -> Tuple[int, int, bool]:
    """One token's bytes entered with the text ending in an odd (escaped) or even run of backslashes -> (need, delta, escaped at its end):
    an unescaped '{' opens and an unescaped '}' closes; need = how far the token dips below its entry depth, delta = its net change.
    Braces and the backslash are ASCII, so UTF-8 continuation bytes never look like one."""
    rel = low = 0
    for c in data:
        if c == 0x5C:
            escaped = not escaped
            continue
        if not escaped:
            if c == 0x7B:
                rel += 1
            elif c == 0x7D:
                rel -= 1
                low = min(low, rel)
        escaped = False
    return -low, rel, escaped


def brace_rules(tokenizer, depth_max: int = 64, ban: Optional[Sequence[int]] = None, eos: Optional[int] = None,
                vocab: Optional[int] = None) -> TokenRules:
    """The two-state LaTeX rule of a byte-level vocabulary (``tokenizer.vocab``: id -> bytes): state = the text so far ends in an odd run of
    backslashes; a token's need / delta are those of its unescaped braces (token_braces); eos (default: the tokenizer's <EOS>) is
    ONLY_AT_ZERO; the ids of `ban` (default: <BOS> and <PAD>) and every id below `vocab` (default: the tokenizer's size) without a byte string
    are banned, and so is a token whose braces do not fit an entry's fields."""
    special = getattr(tokenizer, "special_tokens", {})
    V = int(vocab) if vocab is not None else max(int(tokenizer.vocab_size), max(tokenizer.vocab) + 1)
    if eos is None:
        eos = special.get("<EOS>")
    if ban is None:
        ban = [special[k] for k in ("<BOS>", "<PAD>") if k in special]
    banned = {int(b) for b in ban}
    table = np.zeros((2, V), dtype=np.int32)
    for s in (0, 1):
        for v in range(V):
            data = tokenizer.vocab.get(v)
            if data is None or v in banned:
                table[s, v] = pack(flags=BAN)
                continue
            need, delta, esc = token_braces(data, bool(s))
            if need > 255 or not -128 <= delta <= 127:
                table[s, v] = pack(next=int(esc), flags=BAN)
                continue
            table[s, v] = pack(need, delta, int(esc), ONLY_AT_ZERO if eos is not None and v == int(eos) else 0)
    return TokenRules(table, depth_max)
