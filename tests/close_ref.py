"""The closing decode (include/texocr.h: txo_set_rules_close) restated for the tests, numpy only.  Holds no tests.

brute_dist is independent of TokenRules.close_dist: a breadth-first search from every node on its own that walks ALL V tokens of a node
through TokenRules.allowed / TokenRules.step, no deduplication and no reversed edges.  The replays apply TokenRules.mask(remaining=, ended=,
dist=) -- the one restatement of the budgeted rule -- to the logits a call returned."""
import numpy as np

from texocr_amd import rules as R


def brute_dist(rules, eos):
    """(S, depth_max + 1) int32: picks, the eos included, from every node to a committed eos over allowed tokens; R.CLOSE_INF: none"""
    S, W, V = rules.n_states, rules.depth_max + 1, rules.vocab
    out = np.full((S, W), int(R.CLOSE_INF), dtype=np.int32)
    for s0 in range(S):
        for d0 in range(W):
            seen, frontier, level = {(s0, d0)}, [(s0, d0)], 0
            while frontier and out[s0, d0] == R.CLOSE_INF:
                level += 1
                nxt = []
                for node in frontier:
                    st = np.asarray([node], dtype=np.int32)
                    ok = rules.allowed(st)[0]
                    if 0 <= eos < V and ok[eos]:
                        out[s0, d0] = level
                        break
                    for v in np.nonzero(ok)[0]:
                        n2 = tuple(int(x) for x in rules.step(st, [v])[0][0])
                        if n2 not in seen:
                            seen.add(n2)
                            nxt.append(n2)
                frontier = nxt
    return out


def closing_counter_rules(V, eos, depth_max, banned=()):
    """tests/test_gpu_rules.py's counter_rules (ids % 5 == 0 open, ids % 5 == 1 close with need 1, two states with next = id & 1, `banned`
    banned) with eos enabled: its entry is (need 0, delta 0, ONLY_AT_ZERO) whatever eos % 5 is -- at V = 64 the eos id 61 would otherwise
    be a close token that needs depth 1 and is allowed at depth 0 only, i.e. never.  The two states are copies on purpose (the counter
    isolates the depth); tests/rule_zoo.py holds the rule sets whose states differ."""
    ids = np.arange(V)
    flags = np.zeros(V, dtype=np.int64)
    flags[np.asarray(sorted(banned), dtype=np.int64)] |= R.BAN
    need, delta = (ids % 5 == 1).astype(np.int64), (ids % 5 == 0).astype(np.int64) - (ids % 5 == 1)
    need[eos], delta[eos], flags[eos] = 0, 0, R.ONLY_AT_ZERO
    row = R.pack(need=need, delta=delta, next=ids & 1, flags=flags)
    return R.TokenRules(np.stack([row, row]), depth_max).validate(V)


def replay(rules, dist, logits, tokens, max_len, close=True):
    """logits (B, n, V) and tokens (B, n) of a call from BOS over max_len positions -> (the masked rows (B, n, V) the selection saw, final
    state (B, 2), ended (B,)), stepping with the engine's tokens; close=False: the plain rule's rows"""
    logits, tokens = np.asarray(logits, dtype=np.float32), np.asarray(tokens)
    B, n, _ = logits.shape
    st, ended = rules.start(B), np.zeros(B, dtype=bool)
    rows = np.empty_like(logits)
    for t in range(n):
        rows[:, t] = rules.mask(st, logits[:, t], remaining=max_len - t, ended=ended, dist=dist) if close else rules.mask(st, logits[:, t])
        st, _ = rules.step(st, tokens[:, t])
        ended = ended | (tokens[:, t] == dist.eos)
    return rows, st, ended


def closed_rows(rules, tokens, eos):
    """per row of tokens (B, n): the row holds an eos, and rules.run up to and including the first one allows every token"""
    out = []
    for row in np.asarray(tokens).tolist():
        out.append(eos in row and bool(rules.run(row[:row.index(eos) + 1])[1].all()))
    return out
