"""Constrained beam search (include/texocr.h: txo_set_rules_beam; csrc/beam_rules.h) on the GPU.

Two references the project already trusts, neither restated: the rule is texocr_amd.rules.TokenRules, and every step of a search is
tests/beam_ref.py's float64 replay -- here with -inf in the float64 log-probabilities wherever the parent's state (rules.run on that beam's
prefix) forbids the token.  The mask adds no arithmetic, so the replay's eps are the unconstrained replay tests' own (imported).  Where
the answer is exact -- allow-all rules against the plain search, a ragged batch against the image alone, rule states against rules.run --
it is compared bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

import beam_ref as br
import rules_ref
from gpu_harness import build, knobs, rgb_images
from test_gpu_beam import _Ref, _eps_bf16, _eps_fp32
from test_gpu_rules import _tiny, counter_rules
from texocr_amd import rules as R
from texocr_amd import synth
from texocr_amd._lib import Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES
from texocr_amd.tokenizer import RegExTokenizer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = 12
_REFS = {}


def _case(vocab, images=2, bias=None, seed=3, max_len=24):
    """(dims, weights, float64 reference) of one tiny model, kept for the module: bias = {tuple of token ids: logit offset}"""
    key = (vocab, images, seed, max_len, tuple(sorted((bias or {}).items())))
    if key not in _REFS:
        d = _tiny(vocab, max_len=max_len)
        sd = synth.synth_state_dict(d, seed)
        if bias:
            b = sd["decoder.net.to_logits.bias"].copy()
            for ids, off in bias.items():
                b[list(ids)] += off
            sd["decoder.net.to_logits.bias"] = b
        _REFS[key] = _Ref(d, sd, rgb_images(images, 48, 64, 40 + images))
    return _REFS[key]


def _model(ref, dtype="fp32", beams=8):
    _, _, m = build(ref.d, sd=ref.sd, dtype=dtype, max_batch=ref.img.shape[0] * beams)
    m.rules_beam = True
    m.eos_token = None
    return m


def _allow_all(V):
    return R.TokenRules(np.zeros((1, V), dtype=np.int32), 1)


def _cut(row, eos):
    row = list(row)
    return row[:row.index(eos) + 1] if eos is not None and eos in row else row


def _masked_logp_of(ref, rules, eos):
    """beam_ref's logp_of under rules: the float64 log-probabilities after every beam's prefix, -inf where the state behind that prefix
    (rules.run up to the prefix's first eos: a finished beam's state is frozen, and the replay lets it offer eos only) forbids the token"""
    def logp_of(tokens):
        tokens = np.asarray(tokens, np.int64)
        B, k, _ = tokens.shape
        state = np.stack([rules.run(_cut(tokens[b, j].tolist(), eos))[0] for b in range(B) for j in range(k)])
        return np.where(rules.allowed(state).reshape(B, k, -1), ref.logp(tokens), -np.inf)
    return logp_of


def _states(m, img, k, lengths, rules, **kw):
    """{n: (tokens (B, k, n), scores (B, k))} and {n: Beams} of one constrained search per length (length_alpha = 0: the search's own order)"""
    out, beams = {}, {}
    for n in lengths:
        res = m.beam_search(img, k, n, rules=rules, **kw)
        assert m._engine.query(Q_LAST_PERSISTENT) == 0
        assert res.rule_state.shape == (img.shape[0], k, 2) and res.rule_state.dtype == torch.int32
        out[res.tokens.shape[2]] = (res.tokens.cpu().numpy(), res.scores.cpu().numpy())
        beams[res.tokens.shape[2]] = res
    return out, beams


def _check_live_beams(rules, res, eos, tag=""):
    """every finite-score beam passes rules.run at every position up to its length, and its rule_state is rules.run's final state: exact"""
    tok, sc, ln, st = (x.cpu().numpy() for x in (res.tokens, res.scores, res.lengths, res.rule_state))
    live = 0
    for b in range(tok.shape[0]):
        for r in range(tok.shape[1]):
            if not np.isfinite(sc[b, r]):
                continue
            live += 1
            row = tok[b, r, :ln[b, r]].tolist()
            assert ln[b, r] == len(_cut(tok[b, r].tolist(), eos)), (tag, b, r)
            want, ok = rules.run(row)
            assert bool(ok.all()), (tag, b, r, row, ok.tolist())
            assert st[b, r].tolist() == want.tolist(), (tag, b, r, st[b, r].tolist(), want.tolist())
    return live


# ---- 1. allow-all rules are the plain search, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("vocab", [64, 67, 1100])
def test_allow_all_rules_are_the_plain_search_bit_for_bit(vocab, dtype):
    """S = 1, every entry 0: tokens, scores, lengths and logp of the constrained kernel are the plain kernel's bits (the same log-sum-exp
    in the same order over the raw row) for k = 1, 3, 8 on both request shapes of the register path and on the general path; every state
    reads (0, 0).  eos is the model's own, so that lengths are not all n where a beam does emit it."""
    ref = _case(vocab, images=3)
    m = _model(ref, dtype)
    m.eos_token = ref.d.eos
    img = ref.img.cuda()
    for k in (1, 3, 8):
        plain = m.beam_search(img, k, 16, return_logp=True)
        ruled = m.beam_search(img, k, 16, return_logp=True, rules=_allow_all(vocab))
        assert plain.rule_state is None and ruled.rule_state.shape == (3, k, 2)
        for name in ("tokens", "scores", "lengths", "logp"):
            assert torch.equal(getattr(plain, name), getattr(ruled, name)), (k, name)
        assert not bool(ruled.rule_state.any())
        best, state = m.generate(img, 16, beam=k, rules=_allow_all(vocab))          # txo_generate_beam under the switch
        assert torch.equal(best, m.generate(img, 16, beam=k)) and state.shape == (3, k, 2) and not bool(state.any())


# ---- 2. every step is the float64 replay -------------------------------------------------------------------------------------------
def _banned_early(free, eos, positions=4):
    """the tokens the free BEST beams hold at their first positions: enough to move the search off its free course, few enough to leave the
    vocabulary of 64 its always-allowed tokens"""
    return set(free.tokens[:, 0, :positions].cpu().numpy().reshape(-1).tolist()) - {eos}


@pytest.mark.parametrize("k,vocab,dtype,lanes", [(1, 64, "fp32", 0), (4, 67, "fp32", 0), (8, 64, "fp32", 0), (4, 1100, "fp32", 0),
                                                 (8, 1100, "bf16", 0), (4, 64, "bf16", 0), (4, 67, "fp32", 2)])
def test_every_step_is_the_float64_replay(k, vocab, dtype, lanes):
    """beam_ref.replay_pairs over ALL positions 0 .. STEPS - 1 with the masked float64 log-probabilities: ancestry, score increments,
    selection, order, ties, and 'dead' where a state leaves fewer finite candidates than beams.  k = 1, 4, 8; V = 64 / 67 (the register
    path's two request shapes) and 1100 (the general path); lanes = 2: two row ranges, forced as test_beam_replay_two_row_ranges does."""
    ref = _case(vocab)
    m = _model(ref, dtype)
    img = ref.img.cuda()
    free = m.beam_search(img, k, STEPS)
    rules = counter_rules(vocab, ref.d.eos, 2, _banned_early(free, ref.d.eos) | {ref.d.bos, ref.d.pad})
    with knobs(TXO_LANES=lanes) if lanes else knobs():
        states, beams = _states(m, img, k, range(1, STEPS + 1), rules, return_logp=True)
        if lanes:
            assert m._engine.query(Q_LAST_ROW_RANGES) == lanes
    assert sorted(states) == list(range(1, STEPS + 1))
    rep = br.replay_pairs(ref.s64, ref.enc64, ref.d.bos, None, states, range(STEPS), _eps_bf16 if dtype == "bf16" else _eps_fp32,
                          logp_of=_masked_logp_of(ref, rules, None))
    print(f"\nconstrained beam replay k = {k}, V = {vocab}, {dtype}, ranges {lanes or 1}: {rep.steps} steps, max |score increment - float64 "
          f"log-prob| {rep.inc_err:.3e}, smallest selection slack {rep.slack:.3e} (float64's own margin {rep.gap:.1e}), ties {rep.ties}")
    assert rep.steps == STEPS
    last = beams[STEPS]
    assert not torch.equal(last.tokens, free.tokens), "the rules never moved the search: nothing was tested"
    assert _check_live_beams(rules, last, None) == 2 * k
    # the increments summed left to right in float32 are the score, bit for bit, under rules as without
    acc = torch.zeros_like(last.scores)
    for t in range(STEPS):
        acc = acc + last.logp[:, :, t]
    assert torch.equal(acc, last.scores)


# ---- 3. the rules bind, by construction --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab,k,depth_max,eos_bias", [(64, 3, 1, 2.0), (64, 3, 8, 2.0), (1100, 4, 1, 1.0), (67, 2, 8, 2.0)])
def test_rules_bind_by_construction(vocab, k, depth_max, eos_bias):
    """as test_gpu_rules._binding_rules: the free search's own tokens are banned (so every free beam violates) + the counter with eos only
    at depth 0; eos is favoured by a logit bias so that beams finish at different lengths (at V = 64 the counter makes eos = 61 a closer
    that is also ONLY_AT_ZERO, so no beam ever finishes there: the cap and the bans alone)"""
    ref = _case(vocab, images=3, bias={(vocab - 3,): eos_bias})
    d = ref.d
    m = _model(ref)
    m.eos_token = d.eos
    img = ref.img.cuda()
    free = m.beam_search(img, k, STEPS)
    banned = set(free.tokens.cpu().numpy().reshape(-1).tolist()) - {d.eos}
    rules = counter_rules(vocab, d.eos, depth_max, banned | {d.bos, d.pad})
    for b in range(3):                                             # vacuity: every image's free best beam violates the rule set
        row = free.tokens[b, 0, :int(free.lengths[b, 0])].tolist()
        assert not bool(rules.run(row)[1].all()), (b, row)
    got = m.beam_search(img, k, STEPS, return_logp=True, rules=rules)
    n = min(got.tokens.shape[2], free.tokens.shape[2])
    assert not torch.equal(got.tokens[:, :, :n], free.tokens[:, :, :n])
    assert _check_live_beams(rules, got, d.eos, "alpha 0") >= 3
    if depth_max == 1:
        assert int(got.rule_state[..., 1].max()) <= 1
    ranked = m.beam_search(img, k, STEPS, return_logp=True, length_alpha=0.7, rules=rules)
    assert _check_live_beams(rules, ranked, d.eos, "alpha 0.7") >= 3
    # the same set of beams in another order: every (tokens, score, state) of one call is in the other
    def rows(res):
        return [sorted((tuple(res.tokens[b, r].tolist()), float(res.scores[b, r]), tuple(res.rule_state[b, r].tolist()))
                       for r in range(k) if bool(torch.isfinite(res.scores[b, r]))) for b in range(3)]
    assert rows(got) == rows(ranked)
    key = ranked.scores.double() / ranked.lengths.double() ** 0.7
    assert bool((key[:, :-1] >= key[:, 1:] - 1e-6).all())
    print(f"\n[beam rules] V = {vocab}, k = {k}, depth_max = {depth_max}: lengths {got.lengths.tolist()}, reordered by length_alpha: "
          f"{not torch.equal(got.tokens, ranked.tokens)}")


# ---- 4. fewer allowed candidates than k --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [64, 1100])
def test_fewer_allowed_candidates_than_beams(vocab):
    """state 0 allows exactly two tokens, state 1 allows all, k = 5: behind position 0 two beams are finite and three are dead (the
    replay's 'dead' check passes: no finite candidate was left), from position 1 on all five are finite"""
    ref = _case(vocab)
    m = _model(ref)
    img = ref.img.cuda()
    two = (5, 9)
    row0 = R.pack(next=np.ones(vocab, np.int64), flags=np.where(np.isin(np.arange(vocab), two), 0, R.BAN))
    rules = R.TokenRules(np.stack([row0, R.pack(next=np.ones(vocab, np.int64))]), 1).validate(vocab)
    states, beams = _states(m, img, 5, range(1, 5), rules)
    s1 = states[1][1]
    assert np.isfinite(s1).tolist() == [[True, True, False, False, False]] * 2
    assert all(sorted(states[1][0][b, :2, 0].tolist()) == list(two) for b in range(2))
    rep = br.replay_pairs(ref.s64, ref.enc64, ref.d.bos, None, states, range(4), _eps_fp32, logp_of=_masked_logp_of(ref, rules, None))
    assert rep.steps == 4
    for n in (2, 3, 4):
        assert bool(np.isfinite(states[n][1]).all()), n
        assert bool(np.isin(states[n][0][:, :, 0], two).all()), n
        assert _check_live_beams(rules, beams[n], None) == 10


# ---- 5. eos only at depth 0 ----------------------------------------------------------------------------------------------------------
def test_eos_only_at_depth_zero():
    """eos is a token the free best beam emits while the counter's depth is > 0 (asserted): under the rules every finished beam stands at
    depth 0 in front of its eos, repeated eos leaves score and state as they are, and the search still ends early"""
    V, k, N, eos = 64, 3, 20, 7
    # openers, closers and the eos-to-be favoured: the depth moves, comes back to 0, and token 7 is frequent
    ref = _case(V, images=2, bias={tuple(range(0, 60, 5)): 0.5, tuple(range(1, 60, 5)): 2.0, (eos,): 4.0})
    m = _model(ref)
    img = ref.img.cuda()
    free = m.beam_search(img, k, N)                                # eos_token None: the free beams run on behind token 7
    loose = counter_rules(V, ref.d.eos, 8)
    row = free.tokens[0, 0].tolist()
    depth_before = [int(loose.run(row[:p])[0][1]) for p in range(N)]
    at = [p for p in range(N) if depth_before[p] > 0 and row[p] == eos]
    assert at, (row, depth_before)                                 # such a position exists
    m.eos_token = eos                                              # (the model's own eos id plays no part from here on)
    rules = counter_rules(V, eos, 8)
    assert not bool(rules.run(row[:at[0] + 1])[1].all())           # the free best beam's prefix up to that eos violates the rule set
    states, beams = _states(m, img, k, range(1, N + 1), rules, return_logp=True)
    last_n = max(states)
    got = beams[last_n]
    finished = 0
    for b in range(2):
        for r in range(k):
            if not bool(torch.isfinite(got.scores[b, r])):
                continue
            toks = got.tokens[b, r].tolist()
            if eos in toks:
                finished += 1
                p = toks.index(eos)
                assert int(rules.run(toks[:p])[0][1]) == 0, (b, r, toks)
                assert int(got.lengths[b, r]) == p + 1 and got.rule_state[b, r].tolist() == rules.run(toks[:p + 1])[0].tolist()
                assert all(t == eos for t in toks[p:]) and bool((got.logp[b, r, p + 1:] == 0).all())
    assert finished >= 1
    # every step replayed, finished beams frozen at their score (the replay's 'finished' check), none skipped
    rep = br.replay_pairs(ref.s64, ref.enc64, ref.d.bos, eos, states, range(last_n), _eps_fp32, logp_of=_masked_logp_of(ref, rules, eos))
    assert rep.steps == last_n
    # a finished beam's state does not move while it repeats eos: the same beam at every later length
    for n in range(1, last_n):
        a, b2 = beams[n], beams[n + 1]
        for b in range(2):
            for r in range(k):
                ta = a.tokens[b, r].tolist()
                if eos in ta and bool(torch.isfinite(a.scores[b, r])):
                    same = [q for q in range(k) if b2.tokens[b, q, :n].tolist() == ta and int(b2.tokens[b, q, n]) == eos]
                    assert same and any(torch.equal(b2.rule_state[b, q], a.rule_state[b, r]) and torch.equal(b2.scores[b, q], a.scores[b, r])
                                        for q in same), (n, b, r)
    # the early end: the search stops at the position at which the last beam finished, and asking for more positions changes nothing
    all_done = all(eos in got.tokens[b, r].tolist() or not bool(torch.isfinite(got.scores[b, r])) for b in range(2) for r in range(k))
    print(f"\n[beam rules] eos = {eos} (free best beam emits it at position {at[0]}, depth {depth_before[at[0]]}): constrained search ran "
          f"{last_n} of {N} positions, lengths {got.lengths.tolist()}")
    assert all_done and last_n < N and last_n == int(got.lengths.max())
    more = m.beam_search(img, k, N + 4, return_logp=True, rules=rules)
    for name in ("tokens", "scores", "lengths", "logp", "rule_state"):
        assert torch.equal(getattr(more, name), getattr(got, name)), name
    # a final order that does move (short beams behind long ones): the states move with their tokens
    ranked = m.beam_search(img, k, N, return_logp=True, length_alpha=2.0, rules=rules)
    assert _check_live_beams(rules, ranked, eos) == _check_live_beams(rules, got, eos)
    assert not torch.equal(ranked.tokens, got.tokens)


# ---- 6. ragged -------------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_equals_every_image_alone():
    """fp32, two sizes in one list, under rules: beams, scores, logp and rule_state of an image are its solo call's, bit for bit"""
    ref = _case(64)
    m = _model(ref)
    imgs = [rgb_images(1, h, w, 91 + i)[0].cuda() for i, (h, w) in enumerate([(48, 64), (32, 48)])]
    free = m.beam_search(imgs, 4, STEPS)
    rules = counter_rules(64, ref.d.eos, 2, _banned_early(free, ref.d.eos) | {ref.d.bos, ref.d.pad})
    got = m.beam_search(imgs, 4, STEPS, return_logp=True, rules=rules)
    assert not torch.equal(got.tokens, free.tokens)
    for b, im in enumerate(imgs):
        one = m.beam_search(im[None], 4, STEPS, return_logp=True, rules=rules)
        for name in ("tokens", "scores", "lengths", "logp", "rule_state"):
            assert torch.equal(getattr(got, name)[b], getattr(one, name)[0]), (b, name)
        one_list = m.beam_search([im], 4, STEPS, return_logp=True, rules=rules)
        assert torch.equal(one_list.tokens, one.tokens) and torch.equal(one_list.rule_state, one.rule_state)


# ---- 7. switch and refusals ------------------------------------------------------------------------------------------------------------
def test_switch_and_refusals():
    ref = _case(64)
    _, _, m = build(ref.d, sd=ref.sd, max_batch=8)
    m.eos_token = None
    eng = m._engine
    img = ref.img.cuda()
    assert m.rules_beam is False and eng.rules_beam is False
    off = m.beam_search(img, 4, STEPS, return_logp=True)
    off3 = m.generate(img, STEPS, beam=4, return_beams=True)
    with pytest.raises(ValueError, match="rules_beam must be False or True"):
        m.rules_beam = 2
    m.rules_beam = True
    assert m.rules_beam is True
    on = m.beam_search(img, 4, STEPS, return_logp=True)                     # switch on, no rules: the plain kernels
    assert on.rule_state is None
    for name in ("tokens", "scores", "lengths", "logp"):
        assert torch.equal(getattr(on, name), getattr(off, name)), name
    on3 = m.generate(img, STEPS, beam=4, return_beams=True)
    assert torch.equal(on3[0], off3[0]) and torch.equal(on3[1], off3[1])
    probe = torch.zeros((2, 4, STEPS), dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="txo_last_beam_rule_state: no token rules are set"):
        eng.last_beam_rule_state(probe)
    rules = counter_rules(64, ref.d.eos, 2, _banned_early(off, ref.d.eos) | {ref.d.bos, ref.d.pad})
    eng.set_token_rules(rules)
    with pytest.raises(RuntimeError, match="no constrained beam search has run since the token rules were set"):
        eng.last_beam_rule_state(probe)
    m.generate(img, STEPS)                                                   # a constrained generate is no beam search
    with pytest.raises(RuntimeError, match="no constrained beam search has run since the token rules were set"):
        eng.last_beam_rule_state(probe)
    toks, scores, lengths, logp = eng.beam_search(img, 4, STEPS, None)
    state = eng.last_beam_rule_state(toks)
    for bad in (torch.zeros((1, 4, STEPS), dtype=torch.int64, device="cuda"), torch.zeros((2, 3, STEPS), dtype=torch.int64, device="cuda")):
        with pytest.raises(RuntimeError, match="B and beams must be 2 and 4"):
            eng.last_beam_rule_state(bad)
    assert torch.equal(eng.last_beam_rule_state(toks), state)
    eng.set_token_rules(None)
    with pytest.raises(RuntimeError, match="no token rules are set"):
        eng.last_beam_rule_state(probe)
    # the facade's rules= gives the same beams and states, and generate(beam=k) the same in slot order
    res = m.beam_search(img, 4, STEPS, rules=rules)
    assert torch.equal(res.tokens, toks) and torch.equal(res.scores, scores) and torch.equal(res.rule_state, state)
    t3, s3, st3 = m.generate(img, STEPS, beam=4, return_beams=True, rules=rules)
    assert torch.equal(t3, toks) and torch.equal(s3, scores) and torch.equal(st3, state)
    best, st1 = m.generate(img, STEPS, beam=4, rules=rules)
    assert torch.equal(best, toks[:, 0]) and torch.equal(st1, state)
    assert eng.token_rules is None
    # a reload of the weights makes a new handle: the switch follows the engine object
    m.load_state_dict(ref.sd)
    assert torch.equal(m.beam_search(img, 4, STEPS, rules=rules).tokens, toks)
    m.rules_beam = False
    assert torch.equal(m.beam_search(img, 4, STEPS).tokens, off.tokens)


def test_torch_free_c_program(tmp_path):
    """examples/beam_rules_tiny.c: plain C + the HIP runtime API: the refusal with the switch off, the constrained beams with it on,
    txo_last_beam_rule_state, the free beams again without rules"""
    import subprocess
    import sys
    from texocr_amd import build as b
    exe = b.build_example(verbose=False, name="beam_rules_tiny")
    blob = str(tmp_path / "tiny.bin")
    subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), "examples", "make_tiny_blob.py"), blob], check=True, capture_output=True)
    r = subprocess.run([exe, blob], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "switch off: beam search: not available while token rules are set" in r.stdout
    assert "hold none of them" in r.stdout and "are the first run's" in r.stdout


def test_wrapper_balanced_beam(tmp_path):
    """TeXOCRWrapper(config, rules_beam=True, balanced=True) with decode='beam': the tokenizer's brace rule inside the beam selection --
    every best beam that finished is balanced by the byte scan, no returned row dips below depth 0, and the free beams do violate"""
    from PIL import Image
    from texocr_amd.config import default_config
    from texocr_amd.wrapper import TeXOCRWrapper
    v = json.load(open(os.path.join(HERE, "golden", "tokenizer_vocab_1k.json")))
    tk = RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"])
    tk.save(str(tmp_path / "vocab.txt"))
    cfg = default_config(img_size=[64, 256], max_length=32, in_channels=1,
                         encoder={"embed_dim": 64, "heads": 2, "num_layers": 1}, decoder={"embed_dim": 64, "heads": 2, "num_layers": 2})
    cfg["tokenizer_path"] = str(tmp_path / "vocab.txt")
    w = TeXOCRWrapper(cfg, max_batch=9, balanced=True, rules_beam=True)
    assert w.model.rules_beam is True
    sd = synth.synth_state_dict(w.dims, 5)
    b = sd["decoder.net.to_logits.bias"].copy()
    b[[t for t in range(997) if R.token_braces(tk.vocab[t], False)[0] > 0]] += 1.5
    b[w.model.eos_token] += 1.5                                   # (some best beams finish inside 20 positions, the free ones not at once)
    sd["decoder.net.to_logits.bias"] = b
    w.model.load_state_dict(sd)
    rng = np.random.RandomState(0)
    pil = []
    for wd, ht in [(200, 40), (30, 30), (250, 64)]:
        a = np.full((ht, wd, 3), 255, dtype=np.uint8)
        a[rng.randint(0, ht, 40), rng.randint(0, wd, 40)] = rng.randint(0, 120, (40, 1))
        pil.append(Image.fromarray(a))
    eos = w.model.eos_token
    got = w.batch(pil, max_len=20, decode="beam", beams=3)
    one = [w(im, max_len=20, decode="beam", beams=3) for im in pil]
    free = w.batch(pil, max_len=20, decode="beam", beams=3, balanced=False)
    assert [g[0] for g in got] == [o[0] for o in one]
    res = w.model.beam_search(w._images(pil, "host"), 3, 20, rules=w._rules(None, "beam"))
    finished = 0
    for b_, g in enumerate(got):
        full = res.tokens[b_, 0, :int(res.lengths[b_, 0])].tolist()
        assert g[0] == full[:-1]
        s = rules_ref.scan(tk.vocab, full, 64, eos)
        assert s.low >= 0 and not any(s.disallowed), full
        if eos in full:
            finished += 1
            need = delta = 0
            esc = False
            for t in full[:-1]:                                    # rules.token_braces over the returned row: balanced, never below zero
                n_, d_, esc = R.token_braces(tk.vocab[t], esc)
                assert delta - n_ >= 0
                delta += d_
            assert delta == 0 and res.rule_state[b_, 0, 1] == 0, full
    assert finished >= 1, "no best beam finished: nothing was tested"
    assert len(free) == 3
    # vacuity over all the free beams (an image's best free beam may well be balanced): one of them closes a
    # group that is not open, or ends inside one
    loose = w.model.beam_search(w._images(pil, "host"), 3, 20)
    scans = [rules_ref.scan(tk.vocab, loose.tokens[i, r, :int(loose.lengths[i, r])].tolist(), 64, eos) for i in range(3) for r in range(3)]
    print(f"\n[beam rules] wrapper: constrained best beams {[g[0] for g in got]}, free beams' lowest depths {[x.low for x in scans]}")
    assert any(x.low < 0 or any(x.eos_depths) for x in scans), "the free beams are balanced: nothing was tested"
    assert w.model._engine.token_rules is None
