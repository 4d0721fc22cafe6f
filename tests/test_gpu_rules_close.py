"""Closing decode (include/texocr.h: txo_set_rules_close; csrc/step_rules.h, csrc/beam_rules.h, csrc/rules_close.h) on the GPU.

tests/test_gpu_rules.py's pattern: tiny Dims, return_logits=True, every pick replayed on the host with no tolerance -- here with the
budgeted mask, TokenRules.mask(remaining=, ended=, dist=) through tests/close_ref.py.  The rule set is that file's counter with eos
enabled (close_ref.closing_counter_rules), depth_max 8, 20 positions: dist[s][d] = d + 1, dist_max = 9.  Where a path returns no logits a
row is compared with the same image decoded alone with close=True, bit for bit in fp32."""
import numpy as np
import pytest
import torch

import beam_ref as br
import close_ref
from gpu_harness import STOP_ENV, build, knobs, rgb_images, stop_case
from test_gpu_beam import _Ref
from test_gpu_sampler import _check as check_draws
from texocr_amd import rules as R
from texocr_amd import synth
from texocr_amd._lib import Q_LAST_COMPACTIONS, Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES
from texocr_amd.config import Dims

pytestmark = pytest.mark.gpu

STEPS, DEPTH = 20, 8


def _tiny(vocab, max_len=24):
    return Dims(canvas=64, in_channels=3, embed_dim=64, enc_heads=2, enc_layers=1, dec_heads=2, dec_layers=2, vocab=vocab,
                max_len=max_len, bos=vocab - 2, eos=vocab - 3, pad=vocab - 1)


def _rules(d, depth_max=DEPTH, banned=()):
    rules = close_ref.closing_counter_rules(d.vocab, d.eos, depth_max, set(banned) | {d.bos, d.pad})
    dist = rules.close_dist(d.eos)
    assert dist.dist_max == depth_max + 1 and not dist.any_inf
    return rules, dist


def _np(x):
    return x.cpu().numpy()


# ---- 1. greedy ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,vocab,B", [("fp32", 64, 3), ("fp32", 67, 1), ("bf16", 64, 1), ("bf16", 67, 3), ("fp32", 1100, 3), ("bf16", 1100, 1)])
def test_greedy_tokens_are_the_budgeted_replay(dtype, vocab, B):
    """tokens = the arg-max of the budgeted mask, rule_state = the replay's, every row holds an eos reached at depth 0, and -- asserted --
    every row differs from the plain rule's replay of the same logits in at least one pick"""
    d, sd, m = build(_tiny(vocab), seed=3, dtype=dtype, max_batch=4)
    img = rgb_images(B, 48, 64, 40 + B).cuda()
    rules, dist = _rules(d)
    toks, logits, state = m.generate(img, STEPS, return_logits=True, rules=rules, close=True)
    assert m._engine.query(Q_LAST_PERSISTENT) == 0
    n = toks.shape[1]
    assert n <= STEPS and logits.shape == (B, n, vocab) and state.shape == (B, 2)
    rows, st, ended = close_ref.replay(rules, dist, _np(logits.float()), _np(toks), STEPS)
    assert np.array_equal(_np(toks), rows.argmax(2))
    assert bool(ended.all()) and all(close_ref.closed_rows(rules, _np(toks), d.eos))
    # the state a call reports is the one behind its last returned position (a row that ended earlier kept picking under the plain rule)
    assert np.array_equal(_np(state), st)
    for r, row in enumerate(_np(toks).tolist()):
        assert rules.run(row[:row.index(d.eos)])[0][1] == 0, r                      # the eos came at depth 0
    plain, _, _ = close_ref.replay(rules, dist, _np(logits.float()), _np(toks), STEPS, close=False)
    moved = (plain.argmax(2) != _np(toks)).any(1)
    assert bool(moved.all()), f"rows {np.nonzero(~moved)[0].tolist()} never met the budget: the test is vacuous for them"
    assert m._engine.token_rules is None                          # rules and switch are gone behind the call


# ---- 2. slack ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,vocab", [("fp32", 64), ("bf16", 67), ("fp32", 1100)])
def test_positions_with_slack_are_the_plain_constrained_decode(dtype, vocab):
    """positions with R - 1 >= dist_max (t <= STEPS - 1 - dist_max): tokens, logits and logp of the closing call are the plain constrained
    call's, bit for bit, greedy and sampled"""
    d, sd, m = build(_tiny(vocab), seed=3, dtype=dtype, max_batch=4)
    img = rgb_images(3, 48, 64, 43).cuda()
    rules, dist = _rules(d)
    n_slack = STEPS - dist.dist_max                               # positions 0 .. n_slack - 1
    assert n_slack == 11
    for kw in (dict(), dict(decode="sample", temp=1.0, seed=5)):
        t0, l0, p0, _ = m.generate(img, STEPS, return_logits=True, return_logp=True, rules=rules, **kw)
        t1, l1, p1, _ = m.generate(img, STEPS, return_logits=True, return_logp=True, rules=rules, close=True, **kw)
        k = min(n_slack, t0.shape[1], t1.shape[1])
        assert k == n_slack, "a row set ended inside the slack: nothing left to compare"
        assert torch.equal(t0[:, :k], t1[:, :k]) and torch.equal(l0[:, :k], l1[:, :k]) and torch.equal(p0[:, :k], p1[:, :k]), kw


# ---- 3. sampled --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,vocab,temp,seed", [("fp32", 1000, 1.0, 7), ("fp32", 67, 0.7, 2 ** 32 + 5), ("fp32", 1030, 1.0, 12), ("bf16", 1000, 0.3, 3)])
def test_every_draw_on_the_budgeted_row(dtype, vocab, temp, seed):
    """the register sampler with 16-byte loads (1000), with one-logit loads (67), the LDS sampler (1030): every draw is sampler_ref's on
    the budgeted masked row; every row ends at an allowed eos.  (Seed 12 at V = 1030: with seed 11 two of the 100 draws fall inside
    check_draws' boundary band, one more than its guard against a case that decides its draws there lets through.)"""
    B = 5
    d, sd, m = build(_tiny(vocab), seed=5, dtype=dtype, max_batch=B)
    img = rgb_images(B, 48, 64, 50).cuda()
    rules, dist = _rules(d)
    toks, logits, state = m.generate(img, STEPS, temp=temp, decode="sample", seed=seed, return_logits=True, rules=rules, close=True)
    n = toks.shape[1]
    rows, st, ended = close_ref.replay(rules, dist, _np(logits.float()), _np(toks), STEPS)
    plain, _, _ = close_ref.replay(rules, dist, _np(logits.float()), _np(toks), STEPS, close=False)
    assert bool((rows != plain).any()), "the budget masked nothing"
    check_draws(f"close V={vocab} {dtype}", _np(toks), rows.reshape(-1, vocab), temp, seed, np.repeat(np.arange(B), n), np.tile(np.arange(n), B))
    assert bool(ended.all()) and all(close_ref.closed_rows(rules, _np(toks), d.eos))
    assert np.array_equal(_np(state), st)


# ---- 4. the engine's table ---------------------------------------------------------------------------------------------------------------
def test_engine_table_is_close_dist():
    import json
    import os
    from texocr_amd.tokenizer import RegExTokenizer
    import test_rules_close_cpu as cpu
    d, sd, m = build(_tiny(64), seed=3, max_batch=1)
    eng = m._engine
    for i, kind in enumerate(("plain", "deep", "banned")):
        rules, eos = cpu.random_rules(np.random.default_rng(300 + i), 3, 64, 4, kind)
        rules = R.TokenRules(np.roll(rules.table, d.eos - eos, axis=1), 4).validate(64)     # (the engine's eos id in place of the table's)
        want = rules.close_dist(d.eos)
        if int(want[0, 0]) == int(R.CLOSE_INF):
            with pytest.raises(ValueError, match="eos is unreachable from the start state"):
                eng.rules_close_dist(rules)
            continue
        assert np.array_equal(eng.rules_close_dist(rules).numpy(), np.asarray(want)), kind
    here = os.path.dirname(os.path.abspath(__file__))
    v = json.load(open(os.path.join(here, "golden", "tokenizer_vocab_1k.json")))
    tk = RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"])
    d, sd, m = build(_tiny(1000), seed=3, max_batch=1)
    brace = R.brace_rules(tk, depth_max=64)
    assert np.array_equal(m._engine.rules_close_dist(brace).numpy(), np.asarray(brace.close_dist(d.eos)))


# ---- 5. forced prefixes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decode", ["greedy", "sample"])
def test_prefix_exact_budget_and_infeasible(decode):
    """a prefix of six open tokens: with exactly seven picks left the row is six closes and an eos; with four picks left it is four closes
    and rule_state reads depth 2.  A second row with a short prefix in the same call is what it is with any other first row."""
    V = 64
    d, sd, m = build(_tiny(V), seed=3, max_batch=2)
    img = rgb_images(2, 48, 64, 95).cuda()
    rules, dist = _rules(d)
    o = 10                                                        # 10 % 5 == 0: an open token
    closes = set(range(1, V, 5)) - {d.eos}
    prefix = torch.tensor([[d.bos] + [o] * 6, [d.bos, 13] + [0] * 5], dtype=torch.int64).cuda()
    kw = dict(decode=decode, temp=1.0, seed=4)
    toks, state = m.generate(img, 7, prefix=prefix, prefix_len=[7, 2], rules=rules, close=True, **kw)
    row = toks[0].tolist()
    assert all(t in closes for t in row[:6]) and row[6] == d.eos, row
    assert state[0, 1].item() == 0
    other7 = toks[1].clone()
    assert all(close_ref.closed_rows(rules, [[13] + toks[1].tolist()], d.eos))
    toks, state = m.generate(img, 4, prefix=prefix, prefix_len=[7, 2], rules=rules, close=True, **kw)
    row = toks[0].tolist()
    assert all(t in closes for t in row) and state[0, 1].item() == 2, (row, state[0].tolist())
    # the second row, with another first row (its own short prefix) in the same call: unaffected by either case, over the columns both
    # calls return up to its eos
    calm = prefix.clone()
    calm[0] = prefix[1]
    for n, want in ((7, other7), (4, toks[1].clone())):
        t2, _ = m.generate(img, n, prefix=calm, prefix_len=[2, 2], rules=rules, close=True, **kw)
        k = min(t2.shape[1], want.shape[0])
        row = want[:k].tolist()
        k = row.index(d.eos) + 1 if d.eos in row else k
        assert k >= 1 and torch.equal(t2[1, :k], want[:k]), n


# ---- 6. paths that return no logits ------------------------------------------------------------------------------------------------------
def test_row_stop_with_compactions_equals_every_image_alone():
    d, sd, img = stop_case()
    _, _, m = build(d, sd=sd, max_batch=40, env=STOP_ENV)
    img = img.cuda()
    rules = close_ref.closing_counter_rules(d.vocab, d.eos, 4, {d.bos, d.pad, 5, 6})
    with knobs(TXO_PERSIST=0):
        toks, state = m.generate(img, 40, stop="row", rules=rules, close=True)
    assert m._engine.query(Q_LAST_COMPACTIONS) >= 1
    n = toks.shape[1]
    assert all(close_ref.closed_rows(rules, _np(toks), d.eos))
    for r in range(0, 40, 3):
        t1, s1 = m.generate(img[r:r + 1], 40, stop="row", rules=rules, close=True)
        k = min(n, t1.shape[1])
        assert torch.equal(toks[r, :k], t1[0, :k]) and bool((toks[r, k:] == d.pad).all()), r
        assert torch.equal(state[r], s1[0]) and state[r, 1].item() == 0, r


def test_captured_steps_two_ranges_and_ragged():
    d, sd, m = build(_tiny(64, max_len=24), seed=3, max_batch=40)
    rules, dist = _rules(d)
    img = rgb_images(3, 48, 64, 90).cuda()
    with knobs(TXO_GRAPH=1):
        tg, lg, sg = m.generate(img, STEPS, return_logp=True, rules=rules, close=True)
        tp, _ = m.generate(img, STEPS, rules=rules)               # the plain constrained step is another captured step
        t12, l12, s12 = m.generate(img, 12, return_logp=True, rules=rules, close=True)   # the same captured step, another end position
    with knobs(TXO_GRAPH=0):
        te, le, se = m.generate(img, STEPS, return_logp=True, rules=rules, close=True)
        tq, _ = m.generate(img, STEPS, rules=rules)
        e12, m12, r12 = m.generate(img, 12, return_logp=True, rules=rules, close=True)
    assert torch.equal(tg, te) and torch.equal(lg, le) and torch.equal(sg, se) and torch.equal(tp, tq)
    assert torch.equal(t12, e12) and torch.equal(l12, m12) and torch.equal(s12, r12)
    assert all(close_ref.closed_rows(rules, _np(te), d.eos)) and all(close_ref.closed_rows(rules, _np(e12), d.eos))
    assert not torch.equal(tp[:, :te.shape[1]], te)
    for r in range(3):
        t1, l1, s1 = m.generate(img[r:r + 1], STEPS, return_logp=True, rules=rules, close=True)
        k = min(te.shape[1], t1.shape[1])
        assert torch.equal(te[r, :k], t1[0, :k]) and torch.equal(le[r, :k], l1[0, :k]), r
    # two row ranges
    img40 = rgb_images(40, 32, 48, 81).cuda()
    with knobs(TXO_LANES=2):
        toks, logp, state = m.generate(img40, 12, return_logp=True, rules=rules, close=True)
        assert m._engine.query(Q_LAST_ROW_RANGES) == 2
    assert all(close_ref.closed_rows(rules, _np(toks), d.eos))
    for r in (0, 19, 20, 39):
        t1, l1, s1 = m.generate(img40[r:r + 1], 12, return_logp=True, rules=rules, close=True)
        k = min(toks.shape[1], t1.shape[1])
        assert torch.equal(toks[r, :k], t1[0, :k]) and torch.equal(logp[r, :k], l1[0, :k]), r
    # a ragged list of three sizes
    imgs = [rgb_images(1, h, w, 91 + i)[0].cuda() for i, (h, w) in enumerate([(32, 64), (48, 48), (16, 32)])]
    tr, lr, srg = m.generate_ragged(imgs, 12, return_logp=True, rules=rules, close=True)
    assert all(close_ref.closed_rows(rules, _np(tr), d.eos))
    for r, im in enumerate(imgs):
        t1, l1, s1 = m.generate(im[None], 12, return_logp=True, rules=rules, close=True)
        k = min(tr.shape[1], t1.shape[1])
        assert torch.equal(tr[r, :k], t1[0, :k]) and torch.equal(lr[r, :k], l1[0, :k]), r


# ---- 7. beam search ----------------------------------------------------------------------------------------------------------------------
_REFS = {}


def _beam_case(vocab):
    if vocab not in _REFS:
        d = _tiny(vocab)
        _REFS[vocab] = _Ref(d, synth.synth_state_dict(d, 3), rgb_images(2, 48, 64, 42))
    return _REFS[vocab]


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("vocab", [64, 1100])
def test_closing_beam_search_is_the_float64_search(k, vocab):
    """12 positions, rules_beam on; V = 64: the register path, 1100: the LDS path.  The reference is beam_ref.search64 -- the float64 search
    that keeps every step -- over the float64 log-probabilities with the budgeted mask (R = 12 - n for the beams of length n): the engine's
    final beams are its final beams, scores within the replay's fp32 bound.  Every live beam is finished at depth 0, lengths <= 12; with
    close left off the call is the plain constrained search bit for bit."""
    N = 12
    ref = _beam_case(vocab)
    d = ref.d
    _, _, m = build(d, sd=ref.sd, max_batch=2 * k)
    m.rules_beam = True
    img = ref.img.cuda()
    rules, dist = _rules(d)

    def logp_of(tokens):
        tokens = np.asarray(tokens, np.int64)
        B, kk, n = tokens.shape
        flat = tokens.reshape(B * kk, n).tolist()
        cut = [row[:row.index(d.eos) + 1] if d.eos in row else row for row in flat]
        state = np.stack([rules.run(row)[0] for row in cut])
        ended = np.array([d.eos in row for row in flat])
        ok = rules.allowed(state, remaining=N - n, ended=ended, dist=dist)
        return np.where(ok.reshape(B, kk, -1), ref.logp(tokens), -np.inf)

    want = br.search64(logp_of, 2, k, d.eos, N)
    res = m.beam_search(img, k, N, rules=rules, close=True, return_logp=True)
    assert m._engine.query(Q_LAST_PERSISTENT) == 0
    tok, sc, ln, st = (_np(x) for x in (res.tokens, res.scores, res.lengths, res.rule_state))
    n = tok.shape[2]
    assert n <= N and n in want                                   # (a dead beam holds the float64 search open, not the engine's)
    wt, ws = want[n]
    live = np.isfinite(sc)
    assert live.any(1).all() and np.array_equal(live, np.isfinite(ws))
    assert np.array_equal(tok[live], wt[live])
    assert float(np.abs(sc[live] - ws[live]).max()) < br.eps_fp32(sc[live])
    for b in range(2):
        for r in range(k):
            if live[b, r]:
                row = tok[b, r, :ln[b, r]].tolist()
                assert ln[b, r] <= N and row[-1] == d.eos and d.eos not in row[:-1], (b, r, row)
                fin, ok = rules.run(row)
                assert bool(ok.all()) and fin[1] == 0 and st[b, r].tolist() == fin.tolist(), (b, r)
    plain = m.beam_search(img, k, N, rules=rules, return_logp=True)
    off = m.beam_search(img, k, N, rules=rules, close=False, return_logp=True)
    for name in ("tokens", "scores", "lengths", "logp", "rule_state"):
        assert torch.equal(getattr(plain, name), getattr(off, name)), name
    assert not torch.equal(plain.tokens[..., :n], res.tokens), "the budget never moved the search"
    best, state = m.generate(img, N, beam=k, rules=rules, close=True)                   # txo_generate_beam
    assert torch.equal(best[:, :n], res.tokens[:, 0])


# ---- 8. refusals and scope ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_scope():
    V = 64
    d, sd, m = build(_tiny(V), seed=3, max_batch=4)
    eng = m._engine
    img = rgb_images(2, 48, 64, 99).cuda()
    rules, dist = _rules(d)
    plain_t, plain_s = m.generate(img, STEPS, rules=rules)
    free = m.generate(img, STEPS)

    def knob(on):
        torch.ops.texocr.set_rules_close(eng.id, on)
    with pytest.raises(ValueError, match="txo_set_rules_close: on must be 0 or 1"):
        from texocr_amd import _lib
        _lib.check(eng.lib.txo_set_rules_close(eng.handle, 2))
    with pytest.raises(ValueError, match="close=True needs rules="):
        m.generate(img, STEPS, close=True)
    with pytest.raises(ValueError, match="close=True needs rules="):
        m.beam_search(img, 2, 8, close=True)
    # eos unreachable: banned everywhere (the counter's eos entry banned); in either order, and nothing changes
    dead = R.TokenRules(rules.table.copy(), DEPTH)
    dead.table[:, d.eos] = R.pack(flags=R.BAN)
    with pytest.raises(ValueError, match="closing decode: eos is unreachable from the start state"):
        m.generate(img, STEPS, rules=dead, close=True)            # rules first, then the switch
    assert eng.token_rules is None
    knob(True)
    try:
        eng.set_token_rules(rules)
        with pytest.raises(ValueError, match="closing decode: eos is unreachable from the start state"):
            eng.set_token_rules(dead)                             # the switch first, then the rules: the installed set stays
        by_hand = eng.generate(img, STEPS, d.eos)                 # switch and rules set by hand: the closing decode
        assert all(close_ref.closed_rows(rules, _np(by_hand), d.eos))
        with pytest.raises(ValueError, match="needs eos = %d, the engine's eos id; got -1" % d.eos):
            eng.generate(img, STEPS, None)
        with pytest.raises(ValueError, match="beam search: not available while token rules are set"):
            m.beam_search(img, 2, 8)
    finally:
        eng.set_token_rules(None)
        knob(False)
    deep = R.TokenRules(rules.table.copy(), DEPTH)                # eos only behind three forced tokens: state 0 has no eos, tokens of state 1 ...
    deep.table[0, d.eos] = R.pack(flags=R.BAN)
    assert int(deep.close_dist(d.eos)[0, 0]) == 2
    with pytest.raises(ValueError, match="needs 2 picks to reach eos from the start state, but the call has 1"):
        m.generate(img, 1, rules=deep, close=True)
    m.rules_beam = True
    with pytest.raises(ValueError, match="beam search: a closing decode needs 2 picks to reach eos from the start state, but the call has 1"):
        m.beam_search(img, 2, 1, rules=deep, close=True)
    with pytest.raises(ValueError, match=r"beams in \[1, 8\]"):
        m.beam_search(img, 9, 1, rules=deep, close=True)          # the entry's own refusals come first
    m.rules_beam = False
    with pytest.raises(RuntimeError, match="no table"):
        from texocr_amd import ops
        ops.rules_close_dist(eng.id, 2, DEPTH)
    # close=False calls answer as before, and everything is back behind the closing calls
    t2, s2 = m.generate(img, STEPS, rules=rules, close=False)
    assert torch.equal(t2, plain_t) and torch.equal(s2, plain_s)
    assert torch.equal(m.generate(img, STEPS), free) and eng.token_rules is None


def test_torch_free_c_program(tmp_path):
    """examples/rules_close_tiny.c: plain C + the HIP runtime API, bytes to a closed row"""
    import os
    import subprocess
    import sys
    from texocr_amd import build as b
    exe = b.build_example(verbose=False, name="rules_close_tiny")
    blob = str(tmp_path / "tiny.bin")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, os.path.join(root, "examples", "make_tiny_blob.py"), blob], check=True, capture_output=True)
    r = subprocess.run([exe, blob], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "every row closed" in r.stdout and "ended open" in r.stdout
