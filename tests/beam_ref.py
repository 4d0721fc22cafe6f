"""One step of beam search replayed in float64 (csrc/step.h: beam_select_kernel, beam_backtrack_kernel; the definition is the one
oracle/cpu_ref.py: beam_search_cached states).  No GPU code and no tests: imported like ref64 and sampler_ref.

generate(img, n, beam=k, return_beams=True) returns the k beams and their scores as they stand after n positions; the decode is
deterministic and slot order is score order.  So two calls at lengths n and n + 1 show ONE step, and every decision of that step can
be checked against a float64 restatement that starts from the engine's own state at n -- no drift accumulates, and no decision has
to be reproduced where float64 itself decides by less than a rounding:

- ancestry: the first n tokens of every beam at n + 1 are one of the k beams at n (several identical ones: the lowest index);
- score increment: score_{n+1}[r] - score_n[parent] is the float64 log_softmax of the parent's prefix at the chosen token within eps
  (a finished parent contributes only eos, at + 0);
- selection: with the float64 candidates score_n[j] + logp64[j][v] (finished beams frozen), every chosen candidate is >= the best
  unchosen one - 2 eps, the chosen scores do not increase, no (parent, token) pair is chosen twice, no -inf candidate is chosen while
  a finite one is left, and among bit-equal scores the flat index parent * V + token ascends;
- finished: a beam that contains eos repeats eos with its score unchanged, bit for bit.

A thin margin between two candidates never makes a step unverifiable: both choices pass.  Nothing is skipped."""
from typing import NamedTuple

import numpy as np
import torch

import ref64

CHECKS = ("shape", "ancestry", "finished", "dead", "increment", "duplicate", "order", "tie", "selection")


class ReplayError(AssertionError):
    """a step the replay rejects; .check names the rule (one of CHECKS)"""

    def __init__(self, check, where, what):
        assert check in CHECKS
        super().__init__(f"beam replay [{check}] {where}: {what}")
        self.check = check


class StepReport(NamedTuple):
    inc_err: float        # max |score increment - float64 log-probability| over the live parents' beams (0.0 if there is none)
    slack: float          # min (float64 chosen candidate - best float64 unchosen candidate); +inf where nothing finite is left unchosen
    ties: int             # pairs of adjacent beams at n + 1 whose finite scores are bit-equal
    gap: float            # the float64 restatement's own margin: min difference of adjacent finite candidates among its top k + 1
    parents: np.ndarray   # (B, k) the beam at n every beam at n + 1 continues


def initial_state(images: int, k: int, dtype=np.float32):
    """the state before position 0: no tokens, beam 0 at score 0, the others dead"""
    s = np.full((images, k), -np.inf, dtype)
    s[:, 0] = 0.0
    return np.zeros((images, k, 0), np.int64), s


def eps_fp32(*scores) -> float:
    """2 x 1e-4 (the fp32 logit bound tests/test_gpu_shapes.py asserts, once for the logit and once for the log-sum-exp) + one fp32
    rounding of the running sum at the largest finite |score| of the given states"""
    m = 0.0
    for s in scores:
        s = _np(s).astype(np.float64)
        f = np.isfinite(s)
        if f.any():
            m = max(m, float(np.abs(s[f]).max()))
    return 2 * 1e-4 + 2.0 ** -23 * m


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def prefix_logp64(s64, enc64, bos: int, tokens) -> np.ndarray:
    """tokens (B, k, n) -> float64 log_softmax over the vocabulary at position n of every beam, (B, k, V): ref64.decoder_net on the
    prefixes [bos, tokens], last position"""
    tokens = _np(tokens).astype(np.int64)
    B, k, n = tokens.shape
    prefix = np.concatenate([np.full((B * k, 1), bos, np.int64), tokens.reshape(B * k, n)], 1)
    lg = ref64.decoder_net(s64, torch.from_numpy(prefix), enc64.repeat_interleave(k, 0))[:, -1]
    return torch.log_softmax(lg.double(), -1).view(B, k, -1).numpy()


def replay_step(s64, enc64, bos, eos, state_n, state_n1, eps, logp64=None) -> StepReport:
    """state_n / state_n1: (tokens (B, k, n) / (B, k, n + 1), scores (B, k)) of two decodes of the same images at lengths n and n + 1
    (n = 0: initial_state).  Raises ReplayError at the first rule a beam breaks; returns the measured maxima otherwise.
    logp64: the (B, k, V) result of prefix_logp64 for state_n's tokens, where the caller already has it."""
    tok_n, sc_n = _np(state_n[0]).astype(np.int64), _np(state_n[1])
    tok_1, sc_1 = _np(state_n1[0]).astype(np.int64), _np(state_n1[1])
    B, k, n = tok_n.shape
    if tok_1.shape != (B, k, n + 1) or sc_n.shape != (B, k) or sc_1.shape != (B, k) or sc_n.dtype != sc_1.dtype:
        raise ReplayError("shape", f"n={n}", f"{tok_n.shape} {sc_n.shape} {sc_n.dtype} -> {tok_1.shape} {sc_1.shape} {sc_1.dtype}")
    if logp64 is None:
        logp64 = prefix_logp64(s64, enc64, bos, tok_n)
    V = logp64.shape[2]
    fin_n = (tok_n == eos).any(2) if eos is not None else np.zeros((B, k), bool)
    s_n, s_1 = sc_n.astype(np.float64), sc_1.astype(np.float64)
    inc_err, slack, ties, gap, parents = 0.0, np.inf, 0, np.inf, np.zeros((B, k), np.int64)
    for b in range(B):
        # float64 candidates from the engine's own scores at n; a finished beam offers eos at its score and nothing else
        cand = s_n[b][:, None] + logp64[b]
        for j in range(k):
            if fin_n[b, j]:
                cand[j] = -np.inf
                cand[j, eos] = s_n[b, j]
        parent, token = np.empty(k, np.int64), tok_1[b, :, n]
        for r in range(k):
            where = f"n={n} image {b} beam {r}"
            match = [j for j in range(k) if np.array_equal(tok_n[b, j], tok_1[b, r, :n])]
            if not match:
                raise ReplayError("ancestry", where, f"prefix {tok_1[b, r, :n].tolist()} is none of the {k} beams at n")
            j = parent[r] = match[0]
            v = int(token[r])
            if not 0 <= v < V:
                raise ReplayError("shape", where, f"token {v} outside the vocabulary of {V}")
            if fin_n[b, j]:
                if v != eos:
                    raise ReplayError("finished", where, f"parent {j} holds eos but the beam goes on with token {v}")
                if sc_1[b, r] != sc_n[b, j]:
                    raise ReplayError("finished", where, f"parent {j} holds eos but the score moved {sc_n[b, j]!r} -> {sc_1[b, r]!r}")
                continue
            if not np.isfinite(s_n[b, j]) or not np.isfinite(s_1[b, r]):
                if np.isfinite(cand).sum() > r:
                    raise ReplayError("dead", where, f"parent {j} at score {sc_n[b, j]!r}, beam at {sc_1[b, r]!r}, with finite candidates left")
                continue
            e = abs((s_1[b, r] - s_n[b, j]) - logp64[b, j, v])
            inc_err = max(inc_err, float(e))
            if not e <= eps:
                raise ReplayError("increment", where, f"score {sc_n[b, j]!r} -> {sc_1[b, r]!r} by token {v} of parent {j}: increment "
                                  f"{s_1[b, r] - s_n[b, j]:.9g}, float64 log-probability {logp64[b, j, v]:.9g}, |d| {e:.3g} > eps {eps:.3g}")
        parents[b] = parent
        top = np.sort(cand, axis=None)[::-1][:k + 1]
        top = top[np.isfinite(top)]
        if top.size > 1:
            gap = min(gap, float((top[:-1] - top[1:]).min()))
        flat = parent * V + token
        if len(set(flat.tolist())) != k:
            raise ReplayError("duplicate", f"n={n} image {b}", f"(parent, token) pairs {list(zip(parent.tolist(), token.tolist()))}")
        for r in range(k - 1):
            where = f"n={n} image {b} beams {r}, {r + 1}"
            if not sc_1[b, r] >= sc_1[b, r + 1]:
                raise ReplayError("order", where, f"scores {sc_1[b, r]!r} < {sc_1[b, r + 1]!r}")
            if sc_1[b, r] == sc_1[b, r + 1] and np.isfinite(s_1[b, r]):
                ties += 1
                if not flat[r] < flat[r + 1]:
                    raise ReplayError("tie", where, f"equal scores {sc_1[b, r]!r} but flat indices {int(flat[r])} then {int(flat[r + 1])}")
        chosen = cand[parent, token]
        rest = cand.copy()
        rest[parent, token] = -np.inf
        best_rest = float(rest.max())
        if np.isfinite(best_rest):
            d = float(chosen.min()) - best_rest                       # (-inf where a dead candidate was chosen: rejected below)
            slack = min(slack, d)
            if not d >= -2 * eps:
                r = int(chosen.argmin())
                jj, vv = np.unravel_index(int(rest.argmax()), rest.shape)
                raise ReplayError("selection", f"n={n} image {b} beam {r}", f"chosen (parent {int(parent[r])}, token {int(token[r])}) at float64 "
                                  f"{chosen[r]:.9g} but (parent {jj}, token {vv}) at {best_rest:.9g} was left: {d:.3g} < -2 eps = {-2 * eps:.3g}")
    return StepReport(inc_err, float(slack), ties, float(gap), parents)


class RunReport(NamedTuple):
    steps: int
    inc_err: float
    slack: float
    ties: int
    gap: float
    parents: dict         # n -> (B, k) parents of the beams at n + 1


def replay_pairs(s64, enc64, bos, eos, states: dict, pairs, eps_of, logp_of=None) -> RunReport:
    """states: {n: (tokens, scores)} (n = 0 may be left out: initial_state); replays (n, n + 1) for every n of `pairs`, none skipped;
    eps_of(state_n, state_n1) -> eps of that step; logp_of(tokens) -> what prefix_logp64 gives, where the caller keeps those"""
    pairs = list(pairs)
    inc, slack, ties, gap, done, parents = 0.0, np.inf, 0, np.inf, 0, {}
    for n in pairs:
        b = states[n + 1]
        a = states[n] if n in states else initial_state(*_np(b[1]).shape, dtype=_np(b[1]).dtype)
        rep = replay_step(s64, enc64, bos, eos, a, b, eps_of(a, b), logp64=logp_of(a[0]) if logp_of else None)
        inc, slack, ties, gap, done = max(inc, rep.inc_err), min(slack, rep.slack), ties + rep.ties, min(gap, rep.gap), done + 1
        parents[n] = rep.parents
    assert done == len(pairs)
    return RunReport(done, inc, float(slack), ties, float(gap), parents)


def search64(logp_of, images: int, k: int, eos, max_len: int) -> dict:
    """The definition once more, in float64 and numpy, keeping the state after every position: {n: (tokens, scores)} from n = 0 to where
    the search stops (oracle/cpu_ref.py: beam_search_cached returns the last one only; tests hold the two together).
    logp_of(tokens (B, k, n)) -> (B, k, V) float64 log-probabilities after the prefixes."""
    states = {0: initial_state(images, k, np.float64)}
    for n in range(max_len):
        tok, sc = states[n]
        cand = sc[..., None] + logp_of(tok)
        V = cand.shape[2]
        if eos is not None:
            fin = (tok == eos).any(2)
            cand[fin] = -np.inf
            cand[fin, eos] = sc[fin]
        order = np.argsort(-cand.reshape(images, k * V), axis=1, kind="stable")[:, :k]        # ties: the lower flat index first
        parent, token = order // V, order % V
        new = np.concatenate([np.take_along_axis(tok, parent[..., None], 1), token[..., None]], 2)
        states[n + 1] = (new, np.take_along_axis(cand.reshape(images, k * V), order, 1))
        if eos is not None and bool((new == eos).any(2).all()):
            break
    return states
