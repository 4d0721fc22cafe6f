"""The beam replay (tests/beam_ref.py) checked on its own, no GPU: it accepts every step of the oracle's float64 beam search
(oracle/cpu_ref.py: beam_search_cached) and rejects each kind of wrong step it exists to catch."""
import numpy as np
import pytest
import torch

import beam_ref as br
import ref64
from texocr_amd import synth
from texocr_amd.config import Dims

K, STEPS, EPS = 4, 40, 1e-9
DIMS = Dims(canvas=64, in_channels=3, embed_dim=64, enc_heads=2, enc_layers=1, dec_heads=2, dec_layers=2, vocab=64, max_len=48,
            bos=62, eos=61, pad=63)
EOS_BIAS = 1.0            # on the eos logit: beams finish one after another from position 0 to 26; one image has all four finished from there on
                          # (and goes on repeating eos), the other two keep a live beam to the end, so the oracle runs all 40 positions


class Run:
    def __init__(self, eos):
        sd = synth.synth_state_dict(DIMS, 5)
        if eos is not None:
            b = sd["decoder.net.to_logits.bias"].copy()
            b[eos] += EOS_BIAS
            sd["decoder.net.to_logits.bias"] = b
        self.eos, self.s64 = eos, ref64.sd64(sd)
        self.enc = ref64.encode(self.s64, torch.from_numpy(synth.synth_images(3, 3, 32, 48, seed=3)))
        # the oracle's state after every position: the search is deterministic, so a run of n positions is the first n of a longer one
        self.states = {0: br.initial_state(3, K, np.float64)}
        for n in range(1, STEPS + 1):
            t, s = ref64.beam_search(self.s64, self.enc, DIMS.bos, eos, n, K)
            if t.shape[2] < n:
                break                                                        # every beam finished: the oracle stopped
            assert s.dtype == torch.float64
            self.states[n] = (t.numpy().copy(), s.numpy().copy())
        self.steps = max(self.states)

    def replay(self, n, state_n1=None, state_n=None):
        return br.replay_step(self.s64, self.enc, DIMS.bos, self.eos, state_n or self.states[n], state_n1 or self.states[n + 1], EPS)

    def copy(self, n):
        return self.states[n][0].copy(), self.states[n][1].copy()


@pytest.fixture(scope="module")
def runs():
    return {"no_eos": Run(None), "eos": Run(DIMS.eos)}


@pytest.mark.parametrize("which", ["no_eos", "eos"])
def test_every_step_of_the_float64_oracle_is_accepted(runs, which):
    run = runs[which]
    assert run.steps == STEPS
    reps = [run.replay(n) for n in range(STEPS)]
    inc, slack = max(r.inc_err for r in reps), min(r.slack for r in reps)
    print(f"\n{which}: {len(reps)} steps, max increment error {inc:.2e}, smallest selection slack {slack:.2e}")
    assert len(reps) == STEPS and inc < EPS and slack >= 0.0                 # float64 against float64: the slack is the oracle's own margin
    if which == "eos":
        fin = [(run.states[n][0] == DIMS.eos).any(2) for n in range(1, STEPS + 1)]
        assert fin[-1].any(1).all() and not fin[4].all(1).any()               # finished and live beams side by side in every image ...
        assert fin[-1].all(1).sum() == 1                                     # ... and one image whose beams all repeat eos while the others decode


@pytest.mark.parametrize("which", ["no_eos", "eos"])
def test_the_step_by_step_restatement_is_the_oracle(runs, which):
    """beam_ref.search64 keeps every state of the search; they are the oracle's, tokens exact"""
    run = runs[which]
    states = br.search64(lambda tok: br.prefix_logp64(run.s64, run.enc, DIMS.bos, tok), 3, K, run.eos, STEPS)
    assert sorted(states) == sorted(run.states)
    for n in range(1, STEPS + 1):
        assert np.array_equal(states[n][0], run.states[n][0]), n
        np.testing.assert_allclose(states[n][1], run.states[n][1], rtol=0, atol=1e-10)


def _reject(run, n, state_n1, check):
    with pytest.raises(br.ReplayError) as e:
        run.replay(n, state_n1)
    assert e.value.check in ((check,) if isinstance(check, str) else check), str(e.value)
    run.replay(n)                                                            # the untouched step passes
    return e.value.check


def test_a_prefix_that_comes_from_no_parent_is_rejected(runs):
    run = runs["no_eos"]
    for n, pos in ((17, 0), (17, 16), (39, 20)):
        t, s = run.copy(n + 1)
        t[1, 2, pos] = (t[1, 2, pos] + 1) % DIMS.bos
        _reject(run, n, (t, s), "ancestry")


def test_two_slots_histories_swapped_at_one_position_are_rejected(runs):
    run = runs["no_eos"]
    n, seen = 25, []
    t0 = run.states[n + 1][0]
    for a in range(K):
        for b in range(a + 1, K):
            for pos in np.nonzero(t0[0, a, :n] != t0[0, b, :n])[0]:
                t, s = run.copy(n + 1)
                t[0, a, pos], t[0, b, pos] = t[0, b, pos], t[0, a, pos]
                # where two beams differ in one position only, the swap turns each prefix into the other's parent: then the scores give it away
                seen.append(_reject(run, n, (t, s), ("ancestry", "increment")))
    assert len(seen) >= 8 and seen.count("ancestry") >= 4, seen


@pytest.mark.parametrize("sign", [1, -1])
def test_a_score_off_by_ten_eps_is_rejected(runs, sign):
    run = runs["no_eos"]
    for n in (0, 12, 39):
        t, s = run.copy(n + 1)
        s[2, 0 if sign > 0 else K - 1] += sign * 10 * EPS                     # (the best up, the worst down: the order stays)
        _reject(run, n, (t, s), "increment")


def test_a_chosen_candidate_replaced_by_one_worse_by_a_hundredth_is_rejected(runs):
    run = runs["no_eos"]
    for n in (1, 30):
        t, s = run.copy(n + 1)
        logp = br.prefix_logp64(run.s64, run.enc, DIMS.bos, run.states[n][0])
        b, r = 1, K - 1                                                      # the last slot: the scores stay in order
        parent = next(j for j in range(K) if np.array_equal(run.states[n][0][b, j], t[b, r, :n]))
        cand = run.states[n][1][b, parent] + logp[b, parent]
        taken = {int(t[b, q, n]) for q in range(K) if np.array_equal(t[b, q, :n], t[b, r, :n])}
        worse = [v for v in np.argsort(-cand) if cand[v] <= s[b, r] - 1e-2 and int(v) not in taken]
        t[b, r, n], s[b, r] = worse[0], cand[worse[0]]                        # consistent score: only the choice is wrong
        assert s[b, r] > run.states[n + 1][1][b, r] - 0.5                     # the nearest such candidate, not a far one
        _reject(run, n, (t, s), "selection")


def test_a_finished_beam_that_continues_is_rejected(runs):
    run = runs["eos"]
    n, b, r = next((n, b, r) for n in range(5, STEPS) for b in range(3) for r in range(K)
                   if (run.states[n + 1][0][b, r, :n] == DIMS.eos).any())
    t, s = run.copy(n + 1)
    t[b, r, n] = 7
    _reject(run, n, (t, s), "finished")
    t, s = run.copy(n + 1)
    s[b, r] = np.nextafter(s[b, r], -np.inf)                                  # eos repeated, but not at + 0
    _reject(run, n, (t, s), "finished")


def test_duplicates_dead_beams_and_disorder_are_rejected(runs):
    run = runs["no_eos"]
    t, s = run.copy(13)
    t[0, 3], s[0, 3] = t[0, 2], s[0, 2]                                       # the same (parent, token) twice
    _reject(run, 12, (t, s), "duplicate")
    t, s = run.copy(13)
    t[0, [1, 2]], s[0, [1, 2]] = t[0, [2, 1]], s[0, [2, 1]]                   # right beams, wrong slots
    _reject(run, 12, (t, s), "order")
    t, s = run.copy(1)
    s[1, K - 1] = -np.inf                                                     # a dead beam kept at n = 0 although beam 0 offers 64 live candidates
    _reject(run, 0, (t, s), "dead")


def test_equal_scores_must_come_in_flat_index_order():
    """two tokens with the same logits row, bias and embedding: bit-equal scores; the replay counts them and wants the lower flat index first"""
    sd = synth.synth_state_dict(DIMS, 5)
    s64 = ref64.sd64(sd)
    enc = ref64.encode(s64, torch.from_numpy(synth.synth_images(1, 3, 32, 48, seed=3)))
    a = int(ref64.beam_search(s64, enc, DIMS.bos, None, 1, 1)[0][0, 0, 0])
    a2 = a + 1 if a + 1 < DIMS.eos else a - 1
    for key in ("decoder.net.to_logits.weight", "decoder.net.to_logits.bias", "decoder.net.token_embedding.weight"):
        w = sd[key].copy()
        w[max(a, a2)] = w[min(a, a2)]
        sd[key] = w
    s64 = ref64.sd64(sd)
    states = {0: br.initial_state(1, K, np.float64)}
    for n in (1, 2):
        t, s = ref64.beam_search(s64, enc, DIMS.bos, None, n, K)
        states[n] = (t.numpy().copy(), s.numpy().copy())
    for n in (0, 1):
        rep = br.replay_step(s64, enc, DIMS.bos, None, states[n], states[n + 1], EPS)
        assert rep.ties >= 1
    assert states[1][0][0, :2, 0].tolist() == [min(a, a2), max(a, a2)]
    t, s = states[1][0].copy(), states[1][1].copy()
    t[0, [0, 1]] = t[0, [1, 0]]
    with pytest.raises(br.ReplayError) as e:
        br.replay_step(s64, enc, DIMS.bos, None, states[0], (t, s), EPS)
    assert e.value.check == "tie"
