"""Constrained decode (include/texocr.h: txo_set_token_rules; csrc/step_rules.h) on the GPU.

The reference for every pick is a HOST REPLAY: texocr_amd.rules.TokenRules (the rule in numpy) applied to the logits the engine itself
returned (return_logits=True holds the raw fp32 rows the selection read), so tokens are asserted exactly, in fp32 and in bf16, with no
tolerance: greedy = the arg-max of the masked row (lowest index on ties), sampled = tests/sampler_ref.py on the masked row with
tests/test_gpu_sampler.py's own treatment of draws next to a CDF boundary.  Where a path returns no logits (stop='row' with compaction,
captured steps, a prompted decode) a row is compared with the same image decoded alone under the same rules, bit for bit in fp32."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import rules_ref
import sampler_ref as sr
from gpu_harness import SHAPE_CASES, STOP_ENV, build, knobs, rgb_images, stop_case
from test_gpu_logp import FP32_LOGP, SAME_LOGITS
from test_gpu_sampler import _check as check_draws
from texocr_amd import rules as R
from texocr_amd import synth
from texocr_amd._lib import Q_LAST_COMPACTIONS, Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES
from texocr_amd.config import Dims
from texocr_amd.tokenizer import RegExTokenizer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = 20


def _tiny(vocab, max_len=24):
    return Dims(canvas=64, in_channels=3, embed_dim=64, enc_heads=2, enc_layers=1, dec_heads=2, dec_layers=2, vocab=vocab,
                max_len=max_len, bos=vocab - 2, eos=vocab - 3, pad=vocab - 1)


def counter_rules(V, eos, depth_max, banned=(), eos_at_zero=True):
    """the synthetic counter: ids % 5 == 0 open, ids % 5 == 1 close (need 1), eos only at depth 0, two states with next = id & 1, and
    `banned` ids banned.  The two states are copies on purpose (the counter isolates the depth); tests/rule_zoo.py holds the rule sets whose
    states differ."""
    ids = np.arange(V)
    flags = np.zeros(V, dtype=np.int64)
    if eos_at_zero:
        flags[eos] |= R.ONLY_AT_ZERO
    flags[np.asarray(sorted(banned), dtype=np.int64)] |= R.BAN
    row = R.pack(need=(ids % 5 == 1).astype(np.int64), delta=(ids % 5 == 0).astype(np.int64) - (ids % 5 == 1), next=ids & 1, flags=flags)
    return R.TokenRules(np.stack([row, row]), depth_max).validate(V)


def replay_greedy(rules, logits, tokens, state=None):
    """-> (the host's picks (B, n), final state (B, 2), bound (B, n): the RAW arg-max was disallowed), stepping with the engine's tokens"""
    logits, tokens = logits.float().cpu().numpy(), tokens.cpu().numpy()
    B, n, _ = logits.shape
    st = rules.start(B) if state is None else state
    want, bound = np.zeros((B, n), dtype=np.int64), np.zeros((B, n), dtype=bool)
    for t in range(n):
        want[:, t] = rules.mask(st, logits[:, t]).argmax(1)              # (numpy's arg-max: the first maximum)
        bound[:, t] = ~rules.allowed(st)[np.arange(B), logits[:, t].argmax(1)]
        st, _ = rules.step(st, tokens[:, t])
    return want, st, bound


def masked_rows(rules, logits, tokens):
    """-> (masked logits (B, n, V) as the sampler saw them, final state), stepping with the engine's tokens"""
    logits, tokens = logits.float().cpu().numpy(), tokens.cpu().numpy()
    st = rules.start(logits.shape[0])
    out = np.empty_like(logits)
    for t in range(logits.shape[1]):
        out[:, t] = rules.mask(st, logits[:, t])
        st, _ = rules.step(st, tokens[:, t])
    return out, st


def _gather64(logits, toks):
    return torch.log_softmax(logits.double().cpu(), -1).gather(2, toks.cpu()[..., None])[..., 0]


def _binding_rules(m, d, img, depth_max):
    """decode unconstrained, then ban exactly the tokens that run emitted (so every row's first raw arg-max is disallowed) + the counter"""
    free = m.generate(img, STEPS)
    banned = set(free.cpu().numpy().reshape(-1).tolist()) - {d.eos}
    return counter_rules(d.vocab, d.eos, depth_max, banned), free


# ---- 1. binding by construction, greedy ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,vocab,B,depth_max", [("fp32", 64, 3, 8), ("fp32", 67, 1, 1), ("bf16", 64, 1, 1), ("bf16", 67, 3, 8),
                                                      ("fp32", 1100, 3, 1)])
def test_greedy_tokens_are_the_replay(dtype, vocab, B, depth_max):
    """V % 4 == 0 (16-byte requests on logits and rules) and V % 4 != 0 (scalar), 1100: two chunks of the pass; B = 1 and 3; depth_max = 1:
    the cap binds (a second open token is disallowed)"""
    d, sd, m = build(_tiny(vocab), seed=3, dtype=dtype, max_batch=4)
    m.eos_token = None
    img = rgb_images(B, 48, 64, 40 + B).cuda()
    rules, free = _binding_rules(m, d, img, depth_max)
    toks, logits, state = m.generate(img, STEPS, return_logits=True, rules=rules)
    assert m._engine.query(Q_LAST_PERSISTENT) == 0
    assert toks.shape == (B, STEPS) and logits.shape == (B, STEPS, vocab) and state.shape == (B, 2) and state.dtype == torch.int32
    want, st, bound = replay_greedy(rules, logits, toks)
    assert np.array_equal(toks.cpu().numpy(), want)
    assert bool(bound.any(1).all()), "a row never met a disallowed arg-max: the test is vacuous"
    assert np.array_equal(state.cpu().numpy(), st)
    assert not torch.equal(toks, free)
    if depth_max == 1:
        assert int(st[:, 1].max()) <= 1
        # did the cap decide a pick?  The same replay with depth_max = 8 (same states: the engine's tokens never pass depth 1) differs where
        # an open token was the best of what the other rules leave at depth 1
        loose = R.TokenRules(rules.table, 8)
        cap_bound = int((replay_greedy(loose, logits, toks)[0] != want).sum())
        print(f"\n[rules] {dtype} V={vocab} B={B}: the depth cap decided {cap_bound} of {B * STEPS} picks")
        if B == 3:
            assert cap_bound >= 1
    assert m._engine.token_rules is None                          # the call's rules are gone behind it
    assert torch.equal(m.generate(img, STEPS), free)


# ---- 2. sampled ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,vocab,temp,seed", [("fp32", 1000, 1.0, 7), ("fp32", 67, 0.7, 2 ** 32 + 5), ("fp32", 1030, 1.0, 11),
                                                   ("bf16", 1000, 0.3, 3)])
def test_every_draw_on_the_masked_row(dtype, vocab, temp, seed):
    """the register sampler with 16-byte loads (1000), with one-logit loads (67), and the LDS sampler (1030, beyond the register limit):
    every draw is sampler_ref's on the row with -3.4e38f where the rules disallow"""
    B = 5
    d, sd, m = build(_tiny(vocab), seed=5, dtype=dtype, max_batch=B)
    m.eos_token = None
    img = rgb_images(B, 48, 64, 50).cuda()
    rules, _ = _binding_rules(m, d, img, 2)
    toks, logits, state = m.generate(img, STEPS, temp=temp, decode="sample", seed=seed, return_logits=True, rules=rules)
    assert m._engine.query(Q_LAST_PERSISTENT) == 0
    masked, st = masked_rows(rules, logits, toks)
    assert bool((masked == R.MASKED).any(2).all())
    check_draws(f"rules V={vocab} {dtype}", toks.cpu().numpy(), masked.reshape(-1, vocab), temp, seed, np.repeat(np.arange(B), STEPS),
                np.tile(np.arange(STEPS), B))
    stc = rules.start(B)                                          # every token was allowed where it was drawn
    for t in range(STEPS):
        stc, ok = rules.step(stc, toks[:, t].cpu().numpy())
        assert bool(ok.all()), t
    assert np.array_equal(state.cpu().numpy(), st)


# ---- 3. logp ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decode", ["greedy", "sample"])
@pytest.mark.parametrize("vocab", [200, 203])
def test_logp_is_the_raw_log_softmax(vocab, decode):
    """with rules on, logp is log_softmax of the RAW returned logits at the committed token (test_gpu_logp's SAME_LOGITS) and what score()
    reports for the same tokens (its 2 * FP32_LOGP): a token the rules forced on a row keeps its low probability"""
    d, sd, m = build(dataclasses.replace(SHAPE_CASES["w128"][0], vocab=vocab, bos=vocab - 2, eos=vocab - 3, pad=vocab - 1), seed=3, max_batch=5)
    m.eos_token = None
    img = rgb_images(5, 48, 80, 910).cuda()
    rules, _ = _binding_rules(m, d, img, 2)
    toks, logits, logp, _ = m.generate(img, 14, return_logits=True, return_logp=True, decode=decode, temp=0.7, seed=5, rules=rules)
    assert float(logits.abs().max()) < 16                         # the premise of SAME_LOGITS
    e = float((logp.cpu().double() - _gather64(logits, toks)).abs().max())
    print(f"\n[rules] logp vs raw log_softmax V={vocab} {decode}: max |d| {e:.3e}")
    assert e < SAME_LOGITS, e
    assert not torch.equal(toks, logits.argmax(-1))               # the rules moved picks off the raw arg-max: their logp is not the maximum's
    trg = torch.cat([torch.full((5, 1), d.bos, dtype=torch.int64, device="cuda"), toks], 1)
    s = m.score(img, trg, mask=torch.ones_like(trg, dtype=torch.bool))
    e2 = float((s.logp - logp).abs().max())
    print(f"[rules] logp vs score(): max |d| {e2:.3e}")
    assert e2 < 2 * FP32_LOGP, e2
    toks2, logp2, _ = m.generate(img, 14, return_logp=True, decode=decode, temp=0.7, seed=5, rules=rules)      # without logits_out
    assert torch.equal(toks2, toks) and torch.equal(logp2, logp)


# ---- 4. the null rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [64, 67])
def test_null_rule_is_the_plain_launch_path(vocab):
    """S = 1, all entries 0: the tokens are plain generate()'s and greedy logp is bit for bit the plain launch-path run's (the rule kernels
    make the same pass with the same log-sum-exp calls); sampled: the same draws (the rule kernel's sampled logp comes from a pass of its
    own and is bounded in test 3, not compared by bits)"""
    d, sd, m = build(_tiny(vocab), seed=3, max_batch=3)
    m.eos_token = None
    img = rgb_images(3, 48, 64, 60).cuda()
    null = R.TokenRules(np.zeros((1, vocab), dtype=np.int32), 1)
    with knobs(TXO_PERSIST=0):
        t0, l0 = m.generate(img, STEPS, return_logp=True)
        s0 = m.generate(img, STEPS, decode="sample", temp=1.0, seed=9)
    t1, l1, st = m.generate(img, STEPS, return_logp=True, rules=null)
    assert torch.equal(t0, t1) and torch.equal(l0, l1)
    assert bool((st == 0).all())
    s1, _ = m.generate(img, STEPS, decode="sample", temp=1.0, seed=9, rules=null)
    assert torch.equal(s0, s1)


# ---- 5. the brace rule end to end ------------------------------------------------------------------------------------------------
def _tok1k():
    v = json.load(open(os.path.join(HERE, "golden", "tokenizer_vocab_1k.json")))
    return RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"])


def _brace_violations(tk, d, rows, depth_max):
    """per row: (the byte scan dipped below depth 0 or met an eos above depth 0, <BOS> / <PAD> appear)"""
    out = []
    for row in rows:
        s = rules_ref.scan(tk.vocab, row, depth_max, d.eos)
        out.append((s.low < 0 or any(x != 0 for x in s.eos_depths), d.bos in row or d.pad in row, s))
    return out


@pytest.mark.parametrize("decode", ["greedy", "sample"])
def test_brace_rule_end_to_end(decode):
    """V = 1000 (the golden vocabulary), random weights with a logit bias towards closing braces, eos, <BOS> and <PAD> -- so that the free
    run does violate --, B = 4, 32 positions"""
    tk = _tok1k()
    d = _tiny(1000, max_len=32)
    assert (d.eos, d.bos, d.pad) == (997, 998, 999) == tuple(tk.special_tokens[k] for k in ("<EOS>", "<BOS>", "<PAD>"))
    sd = synth.synth_state_dict(d, 13)
    b = sd["decoder.net.to_logits.bias"].copy()
    closers = [v for v in range(997) if R.token_braces(tk.vocab[v], False)[0] > 0]
    b[closers] += 1.5
    b[[d.eos, d.bos, d.pad]] += 1.0
    sd["decoder.net.to_logits.bias"] = b
    _, _, m = build(d, sd=sd, max_batch=4)
    img = rgb_images(4, 48, 64, 70).cuda()
    rules = R.brace_rules(tk, depth_max=64)
    kw = dict(decode=decode, temp=1.0, seed=21)
    free = m.generate(img, 32, **kw)
    toks, state = m.generate(img, 32, rules=rules, **kw)
    got = _brace_violations(tk, d, toks.cpu().tolist(), 64)
    for r, (unbalanced, special, s) in enumerate(got):
        assert not unbalanced and not special, (r, toks[r].tolist())
        assert state[r].tolist() == [int(s.odd), s.depth], r
    assert any(u or sp for u, sp, _ in _brace_violations(tk, d, free.cpu().tolist(), 64)), "the free run is balanced: nothing was tested"


# ---- 6. every path ---------------------------------------------------------------------------------------------------------------
def _alone(m, img, n, rules, rows, **kw):
    return [m.generate(img[r:r + 1], n, rules=rules, **kw) for r in rows]


def test_row_stop_with_compactions_equals_every_image_alone():
    """gpu_harness.stop_case (rows finish anywhere between position 0 and the end) with a compaction every other position; eos is left free of
    the depth here, so that the rows do finish and the ranges shrink: the states follow their rows through the moves"""
    d, sd, img = stop_case()
    _, _, m = build(d, sd=sd, max_batch=40, env=STOP_ENV)
    img = img.cuda()
    rules = counter_rules(d.vocab, d.eos, 2, banned=(d.bos, d.pad, 5, 6), eos_at_zero=False)
    with knobs(TXO_PERSIST=0):
        toks, state = m.generate(img, 40, stop="row", rules=rules)
    assert m._engine.query(Q_LAST_COMPACTIONS) >= 1 and m._engine.query(Q_LAST_PERSISTENT) == 0
    n = toks.shape[1]
    for r in range(0, 40, 3):
        t1, s1 = m.generate(img[r:r + 1], 40, stop="row", rules=rules)
        k = min(n, t1.shape[1])
        assert torch.equal(toks[r, :k], t1[0, :k]) and bool((toks[r, k:] == d.pad).all()), r
        assert torch.equal(state[r], s1[0]), r
        row = toks[r].tolist()
        st, ok = rules.run(row[:row.index(d.eos) + 1 if d.eos in row else n])      # a finished row froze its state behind its eos
        assert bool(ok.all()) and state[r].tolist() == st.tolist(), r


def test_two_row_ranges():
    """bf16, 129 rows on the K/V form: two ranges (asserted); every pick is the replay of the call's own logits.  fp32, 40 rows forced
    onto two ranges: every row is bit for bit the image alone."""
    d, sd, m = build(_tiny(64), seed=3, dtype="bf16", max_batch=129, latent=0)
    m.eos_token = None
    img = rgb_images(129, 32, 48, 80).cuda()
    rules = counter_rules(64, d.eos, 2, banned=(d.bos, d.pad, 7))
    toks, logits, state = m.generate(img, 12, return_logits=True, rules=rules)
    assert m._engine.query(Q_LAST_ROW_RANGES) == 2
    want, st, bound = replay_greedy(rules, logits, toks)
    assert np.array_equal(toks.cpu().numpy(), want) and np.array_equal(state.cpu().numpy(), st) and bool(bound.any())
    d, sd, m = build(_tiny(64), seed=3, max_batch=40)
    m.eos_token = None
    img = rgb_images(40, 32, 48, 81).cuda()
    with knobs(TXO_LANES=2):
        toks, logp, state = m.generate(img, 12, return_logp=True, rules=rules)
        assert m._engine.query(Q_LAST_ROW_RANGES) == 2
    for r in (0, 19, 20, 39):
        t1, l1, s1 = m.generate(img[r:r + 1], 12, return_logp=True, rules=rules)
        assert torch.equal(toks[r], t1[0]) and torch.equal(logp[r], l1[0]) and torch.equal(state[r], s1[0]), r


def test_captured_steps_ragged_window_and_from_enc():
    d, sd, m = build(_tiny(64, max_len=8), seed=3, max_batch=3)
    m.eos_token = None
    img = rgb_images(3, 48, 64, 90).cuda()
    rules = counter_rules(64, d.eos, 2, banned=(d.bos, d.pad, 9))
    # captured steps on and off
    with knobs(TXO_GRAPH=1):
        tg, lg, sg = m.generate(img, 8, return_logp=True, rules=rules)
    with knobs(TXO_GRAPH=0):
        te, le, se = m.generate(img, 8, return_logp=True, rules=rules)
    assert torch.equal(tg, te) and torch.equal(lg, le) and torch.equal(sg, se)
    for r in range(3):
        t1, l1, s1 = m.generate(img[r:r + 1], 8, return_logp=True, rules=rules)
        assert torch.equal(te[r], t1[0]) and torch.equal(le[r], l1[0]) and torch.equal(se[r], s1[0]), r
    # a second rule set with another depth cap on the same captured step: the step is not the cached one
    tight = counter_rules(64, d.eos, 1, banned=(d.bos, d.pad, 9))
    with knobs(TXO_GRAPH=1):
        t2, s2 = m.generate(img, 8, rules=tight)
    with knobs(TXO_GRAPH=0):
        t3, s3 = m.generate(img, 8, rules=tight)
    assert torch.equal(t2, t3) and torch.equal(s2, s3) and int(s2[:, 1].max()) <= 1
    # the sliding window (beyond the 8-entry table; vocabulary a multiple of 8): the replay, and every image alone
    tw, lw, sw = m.generate(img, 13, return_logits=True, rules=rules)
    assert tw.shape == (3, 13)
    want, st, _ = replay_greedy(rules, lw, tw)
    assert np.array_equal(tw.cpu().numpy(), want) and np.array_equal(sw.cpu().numpy(), st)
    for r in range(3):
        t1, s1 = m.generate(img[r:r + 1], 13, rules=rules)
        assert torch.equal(tw[r], t1[0]) and torch.equal(sw[r], s1[0]), r
    # a ragged batch of three sizes
    imgs = [rgb_images(1, h, w, 91 + i)[0].cuda() for i, (h, w) in enumerate([(32, 64), (48, 48), (16, 32)])]
    tr, lr, srg = m.generate_ragged(imgs, 8, return_logp=True, rules=rules)
    for r, im in enumerate(imgs):
        t1, l1, s1 = m.generate(im[None], 8, return_logp=True, rules=rules)
        assert torch.equal(tr[r], t1[0]) and torch.equal(lr[r], l1[0]) and torch.equal(srg[r], s1[0]), r
    # from encoder rows
    enc = m.encoder(img)
    start = torch.full((3, 1), d.bos, dtype=torch.int64, device="cuda")
    tf, sf = m.decoder.generate(start, None, 8, enc=enc, rules=rules)
    assert torch.equal(tf, te) and torch.equal(sf, se)
    with pytest.raises(ValueError, match="rules= needs the engine's own loop"):
        m.decoder.generate(start, None, 8, enc=enc, rules=rules, mask=torch.tensor([[False]] * 3))


# ---- 7. with a prefix ------------------------------------------------------------------------------------------------------------
def test_prefix_advances_the_state():
    """per-row lengths 1, 3, 5.  Everything is banned but one filler and one close token c (need 1) that a logit bias makes the best pick
    wherever it is allowed: the row whose prefix opens two groups closes exactly two and never a third; the row that starts at BOS never
    closes; a forced token the rules ban is committed all the same.  prefix_logp is the run's without rules, bit for bit."""
    V = 64
    d = _tiny(V)
    sd = synth.synth_state_dict(d, 3)
    c, o, f, x = 11, 10, 13, 17                                   # close (11 % 5 == 1), open (10 % 5 == 0), the filler, a banned token
    b = sd["decoder.net.to_logits.bias"].copy()
    b[c] += 50.0
    sd["decoder.net.to_logits.bias"] = b
    _, _, m = build(d, sd=sd, max_batch=3)
    m.eos_token = None
    img = rgb_images(3, 48, 64, 95).cuda()
    rules = counter_rules(V, d.eos, 4, banned=set(range(V)) - {c, f})
    prefix = torch.tensor([[d.bos, 0, 0, 0, 0], [d.bos, x, f, 0, 0], [d.bos, o, f, o, f]], dtype=torch.int64).cuda()
    for lens in ([1, 3, 5], [3, 3, 5]):                           # shortest prefix 1: every forced token inside the loop; 3: two columns in the start kernel
        pre = prefix.clone()
        if lens[0] == 3:
            pre[0, 1:3] = torch.tensor([o, f])
        toks, logp, plogp, state = m.generate(img, 4, prefix=pre, prefix_len=lens, return_logp=True, rules=rules)
        t0, l0, plogp0 = m.generate(img, 4, prefix=pre, prefix_len=lens, return_logp=True)
        assert torch.equal(plogp, plogp0)
        rows = toks.cpu().tolist()
        assert rows[2][:2] == [c, c] and c not in rows[2][2:], rows[2]
        if lens[0] == 1:
            assert c not in rows[0], rows[0]
        else:
            assert rows[0][0] == c and c not in rows[0][1:], rows[0]
        assert c not in rows[1], rows[1]                          # (its banned forced token has delta 0: nothing is open)
        for r in range(3):
            st, ok = rules.run(pre[r, 1:lens[r]].tolist() + rows[r])
            assert state[r].tolist() == st.tolist(), (lens, r)
            assert bool(ok[lens[r] - 1:].all()), (lens, r)        # every PICKED token was allowed
        assert bool((logp <= 0).all())
    # sampled, with the prefix: a forced position consumes no draw -- the picks behind the prefix are allowed and the state is the replay's
    toks, state = m.generate(img, 4, prefix=prefix, prefix_len=[1, 3, 5], decode="sample", temp=1.0, seed=4, rules=rules)
    for r, n in enumerate([1, 3, 5]):
        st, ok = rules.run(prefix[r, 1:n].tolist() + toks[r].tolist())
        assert state[r].tolist() == st.tolist() and bool(ok[n - 1:].all()), r


# ---- 8. refusals and scope -------------------------------------------------------------------------------------------------------
def test_refusals_and_scope():
    d, sd, m = build(dataclasses.replace(SHAPE_CASES["calib256"][0], vocab=1000, bos=998, eos=997, pad=999), seed=3, max_batch=4)
    m.eos_token = None
    eng = m._engine
    img = rgb_images(2, 64, 64, 99).cuda()
    plain = m.generate(img, 8)
    assert eng.query(Q_LAST_PERSISTENT) == 1

    def install(table, depth_max):
        torch.ops.texocr.set_token_rules(torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)), eng.id, depth_max)

    ok = np.zeros((2, 1000), dtype=np.int32)
    t_next = ok.copy(); t_next[1, 3] = R.pack(next=2)
    t_none = ok.copy(); t_none[1] = R.pack(flags=R.BAN)
    for table, dm, text in [(np.zeros((9, 1000)), 4, r"S is 9; the number of states must be in \[1, 8\]"),
                            (ok, 0, r"depth_max is 0; it must be in \[1, 255\]"), (ok, 256, "depth_max is 256"),
                            (t_next, 4, r"rules\[1\]\[3\] has next = 2, not a state below S = 2"),
                            (t_none, 4, "state 1 has no always-allowed token"),
                            (np.zeros((2, 999)), 4, "V is 999 but the engine's vocabulary has 1000 entries")]:
        with pytest.raises(ValueError, match="token rules: .*" + text):
            install(table, dm)
        assert eng.token_rules is None
    with pytest.raises(RuntimeError, match="no token rules are set"):
        eng.last_rule_state(plain)
    rules = R.ban(1000, set(plain.cpu().numpy().reshape(-1).tolist()))
    eng.set_token_rules(rules)
    with pytest.raises(RuntimeError, match="no generate has run since the token rules were set"):
        eng.last_rule_state(plain)
    eng.set_token_rules(None)
    for call in (lambda: m.generate(img, 8, beam=2, rules=rules), lambda: m.beam_search(img, 2, 8, rules=rules),
                 lambda: m.beam_search([img[0], img[1, :, :32]], 2, 8, rules=rules)):
        with pytest.raises(ValueError, match="beam search: not available while token rules are set"):
            call()
        assert eng.token_rules is None
    assert m.beam_search(img, 2, 8).tokens.shape[:2] == (2, 2)    # ... and available again behind them
    toks, state = m.generate(img, 8, rules=rules)
    assert eng.query(Q_LAST_PERSISTENT) == 0 and not bool(torch.isin(toks, plain).any())
    eng.set_token_rules(rules)
    assert torch.equal(eng.generate(img, 8, None), toks)
    with pytest.raises(ValueError, match=r"B must be in \[1, 2\]"):
        eng.last_rule_state(torch.zeros((3, 8), dtype=torch.int64, device="cuda"))
    assert torch.equal(eng.last_rule_state(toks), state)
    eng.set_token_rules(None)
    again = m.generate(img, 8)
    assert eng.query(Q_LAST_PERSISTENT) == 1 and torch.equal(again, plain)
    # a set installed by hand stays across calls, and a call's rules= puts it back behind itself
    eng.set_token_rules(rules)
    t2, s2 = m.generate(img, 8, rules=R.TokenRules(np.zeros((1, 1000), dtype=np.int32), 1))
    assert torch.equal(t2, plain) and eng.token_rules is not None
    assert torch.equal(m._engine.generate(img, 8, None), toks)
    eng.set_token_rules(None)


def test_torch_free_c_program_under_a_ban_rule(tmp_path):
    """examples/rules_tiny.c: plain C + the HIP runtime API: txo_set_token_rules (a ban rule built from a free run, a refused table, off again)
    and txo_last_rule_state"""
    import subprocess
    import sys
    from texocr_amd import build as b
    exe = b.build_example(verbose=False, name="rules_tiny")
    blob = str(tmp_path / "tiny.bin")
    subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), "examples", "make_tiny_blob.py"), blob], check=True, capture_output=True)
    r = subprocess.run([exe, blob], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "produced none of them" in r.stdout and "no always-allowed token" in r.stdout and "are the first run's" in r.stdout


def test_wrapper_balanced(tmp_path):
    """TeXOCRWrapper(..., balanced=True) / __call__ / batch(balanced=): the tokenizer's brace rule through the facades -- the batch equals the
    per-image calls, every returned row passes the byte scan, and balanced=False on a call switches it off again"""
    from PIL import Image
    from texocr_amd.config import default_config
    from texocr_amd.wrapper import TeXOCRWrapper
    tk = _tok1k()
    tk.save(str(tmp_path / "vocab.txt"))
    cfg = default_config(img_size=[64, 256], max_length=32, in_channels=1,
                         encoder={"embed_dim": 64, "heads": 2, "num_layers": 1}, decoder={"embed_dim": 64, "heads": 2, "num_layers": 2})
    cfg["tokenizer_path"] = str(tmp_path / "vocab.txt")
    w = TeXOCRWrapper(cfg, max_batch=3, balanced=True)
    sd = synth.synth_state_dict(w.dims, 5)
    b = sd["decoder.net.to_logits.bias"].copy()
    b[[v for v in range(997) if R.token_braces(tk.vocab[v], False)[0] > 0]] += 1.5
    sd["decoder.net.to_logits.bias"] = b
    w.model.load_state_dict(sd)
    rng = np.random.RandomState(0)
    pil = []
    for wd, ht in [(200, 40), (30, 30), (250, 64), (100, 17)]:
        a = np.full((ht, wd, 3), 255, dtype=np.uint8)
        a[rng.randint(0, ht, 40), rng.randint(0, wd, 40)] = rng.randint(0, 120, (40, 1))
        pil.append(Image.fromarray(a))
    one = [w(im, max_len=20, decode="greedy", return_logp=True) for im in pil]
    got = w.batch(pil, max_len=20, decode="greedy", return_logp=True)
    free = w.batch(pil, max_len=20, decode="greedy", balanced=False)
    for a, g in zip(one, got):
        assert len(a) == 3 and len(g) == 3 and a[0] == g[0] and a[1] == g[1] and a[2] == g[2]
        s = rules_ref.scan(tk.vocab, g[0], 64, w.model.eos_token)
        assert s.low >= 0 and not any(s.disallowed), g[0]
    assert any(rules_ref.scan(tk.vocab, f[0], 64, w.model.eos_token).low < 0 for f in free), "the free run is balanced: nothing was tested"
    assert w.model._engine.token_rules is None
    with pytest.raises(ValueError, match="balanced=True is not available with decode='beam'"):
        w(pil[0], max_len=20, decode="beam")
