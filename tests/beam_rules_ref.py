"""Constrained beam search (csrc/beam_rules.h) once more in numpy, over a table-driven toy model: the logits after a prefix are a fixed
function of its last token, ``table[last]`` (row V: after the start token).  No GPU code and no tests: tests/test_beam_rules_cpu.py pins
it to brute-force enumeration, tests/test_gpu_beam_rules.py takes its helpers for the replay on the GPU.

The rule itself is texocr_amd.rules.TokenRules -- nothing is restated here but the search:
  every slot carries (s, depth), (0, 0) at the start, only slot 0 live; a live parent's candidate (j, v) is score[j] + logp[j][v] (log_softmax
  of the RAW row) where the parent's state allows v and -inf otherwise; a finished parent offers eos at + 0, unmasked, and keeps its state;
  the k best by score, ties to the lower j * V + v; a slot takes its parent's state advanced by its token; a slot whose candidate is -inf is
  dead: never finished by the eos it may hold, and it does not hold the search open."""
import itertools
from typing import Dict, NamedTuple, Optional

import numpy as np


class State(NamedTuple):
    tokens: np.ndarray      # (k, n) int64
    scores: np.ndarray      # (k,) float64, -inf: dead
    rule_state: np.ndarray  # (k, 2) int32
    finished: np.ndarray    # (k,) bool


def log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def masked_logp(rules, rule_state, logp):
    """logp (k, V) of the beams' prefixes -> the same with -inf where the beam's state forbids the token"""
    return np.where(rules.allowed(rule_state), logp, -np.inf)


def toy_logp(table, tokens):
    """tokens (k, n) -> (k, V) float64 log-probabilities after every prefix: the row of the last token, row V before the first"""
    V = table.shape[1]
    last = tokens[:, -1] if tokens.shape[1] else np.full(tokens.shape[0], V)
    return log_softmax(table[last])


def search(table, rules, k: int, eos: Optional[int], max_len: int) -> Dict[int, State]:
    """{n: State} from n = 0 to where the search stops (every live beam finished, or max_len)"""
    V = table.shape[1]
    sc = np.full(k, -np.inf)
    sc[0] = 0.0
    states = {0: State(np.zeros((k, 0), np.int64), sc, rules.start(k), np.zeros(k, bool))}
    for n in range(max_len):
        st = states[n]
        cand = st.scores[:, None] + masked_logp(rules, st.rule_state, toy_logp(table, st.tokens))
        for j in np.nonzero(st.finished)[0]:
            cand[j] = -np.inf
            cand[j, eos] = st.scores[j]
        order = np.argsort(-cand.reshape(-1), kind="stable")[:k]              # ties: the lower flat index first
        parent, token = order // V, order % V
        score = cand.reshape(-1)[order]
        dead = ~np.isfinite(score)
        nxt, _ = rules.step(st.rule_state[parent], token)
        frozen = st.finished[parent]
        nxt[frozen] = st.rule_state[parent][frozen]
        fin = frozen | ((token == eos) & ~dead if eos is not None else np.zeros(k, bool))
        states[n + 1] = State(np.concatenate([st.tokens[parent], token[:, None]], 1), score, nxt.astype(np.int32), fin)
        if eos is not None and bool((fin | dead).all()):
            break
    return states


def brute_scores(table, rules, eos: Optional[int], n: int) -> Dict[tuple, float]:
    """every sequence of length n -> its score by the definition, each on its own: the sum of the raw log-probabilities of its tokens up to
    and including its first eos, -inf if rules.run disallows one of those or a token behind the first eos is not eos"""
    V = table.shape[1]
    out = {}
    for seq in itertools.product(range(V), repeat=n):
        cut = seq.index(eos) + 1 if eos is not None and eos in seq else n
        ok = all(t == eos for t in seq[cut:]) and bool(rules.run(list(seq[:cut]))[1].all())
        total, last = 0.0, V
        for t in seq[:cut]:
            total += float(log_softmax(table[last])[t])
            last = t
        out[seq] = total if ok else -np.inf
    return out
