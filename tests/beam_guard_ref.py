"""Beam search under the repeat guard (csrc/beam_guard.h) once more in numpy: tests/beam_rules_ref.py's search, over the same table-driven toy
model, with the guard and the yield rule.  No GPU code and no tests: tests/test_beam_guard_cpu.py pins it to brute-force enumeration,
tests/test_gpu_beam_guard.py takes `keep` for the replay on the GPU.

The ban set is tests/guard_ref.py's brute-force restatement on the beam's OWN tokens (those its ancestry committed); the rules are
texocr_amd.rules.TokenRules (rules=None: every token allowed).  Nothing is restated here but the search:
  a live, unfinished parent's candidate (j, v) is score[j] + logp[j][v] (log_softmax of the RAW row) where v is allowed and unbanned for j and
  -inf otherwise; a parent with no token both allowed and unbanned drops its ban at that pick (the yield rule); a finished parent offers
  eos at + 0, unmasked; the k best by score, ties to the lower j * V + v; a slot whose candidate is -inf is dead."""
from typing import Dict, Optional

import numpy as np

import guard_ref
from beam_rules_ref import State, toy_logp


def keep(history, allowed, P, R, eos):
    """the (V,) bool mask of one parent's pick: allowed and unbanned, or, where that is empty, allowed alone -> (mask, ban set, yielded)"""
    allowed = np.asarray(allowed, bool)
    ban = guard_ref.banned(history, P, R, eos)
    free = allowed.copy()
    free[sorted(ban)] = False
    yielded = not free.any()
    return (allowed if yielded else free), ban, yielded


def search(table, rules, guard, k: int, eos: Optional[int], max_len: int) -> Dict[int, State]:
    """{n: State} from n = 0 to where the search stops (every live beam finished, or max_len); guard = (P, R) or None"""
    V = table.shape[1]
    sc = np.full(k, -np.inf)
    sc[0] = 0.0
    start = rules.start(k) if rules is not None else np.zeros((k, 2), np.int32)
    states = {0: State(np.zeros((k, 0), np.int64), sc, start, np.zeros(k, bool))}
    for n in range(max_len):
        st = states[n]
        allowed = rules.allowed(st.rule_state) if rules is not None else np.ones((k, V), bool)
        if guard is not None:
            allowed = np.stack([keep(st.tokens[j].tolist(), allowed[j], guard[0], guard[1], eos)[0] for j in range(k)])
        cand = st.scores[:, None] + np.where(allowed, toy_logp(table, st.tokens), -np.inf)
        for j in np.nonzero(st.finished)[0]:
            cand[j] = -np.inf
            cand[j, eos] = st.scores[j]
        order = np.argsort(-cand.reshape(-1), kind="stable")[:k]              # ties: the lower flat index first
        parent, token = order // V, order % V
        score = cand.reshape(-1)[order]
        dead = ~np.isfinite(score)
        frozen = st.finished[parent]
        if rules is not None:
            nxt, _ = rules.step(st.rule_state[parent], token)
            nxt[frozen] = st.rule_state[parent][frozen]
        else:
            nxt = start.copy()
        fin = frozen | ((token == eos) & ~dead if eos is not None else np.zeros(k, bool))
        states[n + 1] = State(np.concatenate([st.tokens[parent], token[:, None]], 1), score, nxt.astype(np.int32), fin)
        if eos is not None and bool((fin | dead).all()):
            break
    return states
