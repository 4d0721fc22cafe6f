"""Beam search under the repeat guard (include/texocr.h: txo_set_guard_beam; csrc/beam_guard.h) on the GPU.

References the project already trusts, none restated: the ban set is tests/guard_ref.py's brute force on the beam's own tokens, the rules
are texocr_amd.rules.TokenRules, the pick set of one parent is tests/beam_guard_ref.keep (allowed minus banned, or allowed alone where that
is empty), and every step of a search is tests/beam_ref.py's float64 replay with -inf outside the pick set.  The mask adds no arithmetic,
so the replay's eps are the unconstrained replay tests' own (imported).  Where the answer is exact -- a guard that cannot bind against the
search without one, a ragged batch against the image alone, rule states against rules.run -- it is compared bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

import beam_guard_ref as bgr
import beam_ref as br
import close_ref
import guard_ref
from gpu_harness import build, knobs, rgb_images
from test_gpu_beam import _eps_bf16, _eps_fp32
from test_gpu_beam_rules import _allow_all, _case, _check_live_beams, _cut
from texocr_amd import guard
from texocr_amd import rules as R
from texocr_amd import synth
from texocr_amd._lib import Q_LAST_GUARDED, Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES
from texocr_amd.tokenizer import RegExTokenizer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = 14
LOOP = {(5,): 4.0, (9,): 3.5, (12,): 3.0}                         # three favoured tokens: the free search loops on them
LOOP2 = {(5,): 8.0, (9,): 7.5}                                    # two, far ahead of the rest: under (4, 2) the beams run into blocks of 2, 3 and 4 tokens


def _model(ref, dtype="fp32", beams=8, eos=None):
    _, _, m = build(ref.d, sd=ref.sd, dtype=dtype, max_batch=ref.img.shape[0] * beams)
    m.guard_beam = True
    m.rules_beam = True
    m.eos_token = eos
    return m


def _loops(tokens, P, Rr, eos=None):
    """how many rows of tokens (B, k, n) hold a token the guard would have banned"""
    return sum(bool(guard_ref.violations(_cut(row, eos), P, Rr, eos)) for b in tokens.tolist() for row in b)


def _guarded_logp_of(ref, g, rules=None, eos=None, periods=None, yields=None, remaining=None):
    """beam_ref's logp_of under the guard: the float64 log-probabilities after every beam's prefix, -inf outside that beam's pick set
    (beam_guard_ref.keep on the beam's own tokens; allowed = the rules' verdict in the state behind the prefix, every token without rules).
    periods / yields: sets that collect the periods whose ban was in force and the (n, image, beam) at which a ban was dropped"""
    def logp_of(tokens):
        tokens = np.asarray(tokens, np.int64)
        B, k, n = tokens.shape
        lp = ref.logp(tokens)
        out = np.full_like(lp, -np.inf)
        for b in range(B):
            for j in range(k):
                h = tokens[b, j].tolist()
                if rules is None:
                    allowed = np.ones(lp.shape[2], bool)
                else:
                    allowed = rules.allowed(rules.run(_cut(h, eos))[0][None])[0]
                keep, ban, yielded = bgr.keep(h, allowed, g[0], g[1], eos)
                out[b, j][keep] = lp[b, j][keep]
                if periods is not None:
                    periods.update(p for x in ban for p in range(1, g[0] + 1) if guard_ref.ends_in_copies(h + [x], p, g[1] + 1))
                if yields is not None and yielded:
                    yields.add((n, b, j))
        return out
    return logp_of


def _states(m, img, k, lengths, **kw):
    out, beams = {}, {}
    for n in lengths:
        res = m.beam_search(img, k, n, **kw)
        assert m._engine.query(Q_LAST_PERSISTENT) == 0 and m._engine.query(Q_LAST_GUARDED) == 1
        out[res.tokens.shape[2]] = (res.tokens.cpu().numpy(), res.scores.cpu().numpy())
        beams[res.tokens.shape[2]] = res
    return out, beams


def _same(a, b, names=("tokens", "scores", "lengths", "logp"), tag=""):
    for name in names:
        assert torch.equal(getattr(a, name), getattr(b, name)), (tag, name)


# ---- 1. switch and refusals ----------------------------------------------------------------------------------------------------------------
def test_switch_and_refusals():
    ref = _case(64, bias=LOOP)
    _, _, m = build(ref.d, sd=ref.sd, max_batch=8)
    m.eos_token = None
    eng = m._engine
    img = ref.img.cuda()
    g = (2, 1)
    assert m.guard_beam is False and eng.guard_beam is False
    off = m.beam_search(img, 4, STEPS, return_logp=True)
    ragged = [img[0], img[1, :, :32]]
    calls = (lambda: m.generate(img, 8, beam=2, repeat_guard=g), lambda: m.beam_search(img, 2, 8, repeat_guard=g),
             lambda: m.beam_search(ragged, 2, 8, repeat_guard=g))

    def refused():
        for call in calls:
            with pytest.raises(ValueError, match="beam search: not available while a repeat guard is set"):
                call()
        assert eng.repeat_guard is None
    refused()
    with pytest.raises(ValueError, match="guard_beam must be False or True"):
        m.guard_beam = 2
    with pytest.raises(ValueError, match="guard_beam must be False or True"):
        m.guard_beam = "on"
    m.guard_beam = True
    assert m.guard_beam is True and eng.guard_beam is True
    on = m.beam_search(img, 4, STEPS, return_logp=True)                      # switch on, no guard: the plain kernels
    _same(on, off)
    assert eng.query(Q_LAST_GUARDED) == 0
    for call in calls:
        call()
        assert eng.query(Q_LAST_GUARDED) == 1 and eng.repeat_guard is None
    got = m.beam_search(img, 4, STEPS, return_logp=True, repeat_guard=g)
    assert _loops(off.tokens, *g) > 0 and _loops(got.tokens, *g) == 0
    # rules beside the guard need rules_beam as ever: the rules' refusal, whatever guard_beam says
    rules = _allow_all(64)
    assert m.rules_beam is False
    with pytest.raises(ValueError, match="beam search: not available while token rules are set"):
        m.beam_search(img, 2, 8, rules=rules, repeat_guard=g)
    m.rules_beam = True
    assert m.beam_search(img, 2, 8, rules=rules, repeat_guard=g).rule_state.shape == (2, 2, 2)
    # generate(close=True, repeat_guard=) outside beam search stays refused in both settings
    crules = close_ref.closing_counter_rules(64, ref.d.eos, 8, {ref.d.bos, ref.d.pad})
    m.eos_token = ref.d.eos
    for setting in (True, False):
        m.guard_beam = setting
        with pytest.raises(ValueError, match="repeat guard: not available with a closing decode"):
            m.generate(img, 12, rules=crules, close=True, repeat_guard=g)
    m.eos_token = None
    # a reload of the weights makes a new handle: the switch follows the engine object
    m.guard_beam = True
    m.load_state_dict(ref.sd)
    _same(m.beam_search(img, 4, STEPS, return_logp=True, repeat_guard=g), got)
    m.guard_beam = False
    refused()
    _same(m.beam_search(img, 4, STEPS, return_logp=True), off)


# ---- 2. a guard that cannot bind is the plain search, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("vocab", [64, 67, 1100])
def test_a_guard_that_cannot_bind_is_the_plain_search_bit_for_bit(vocab, dtype):
    """guard (16, 16) over 16 positions: the smallest history with a ban has R * 1 = 16 tokens and the last pick has 15 (guard.hits on a
    constant row of 16 is empty).  Tokens, scores, lengths and logp of the guarded kernel are those of beam_select_kernel without rules, of
    beam_select_rules_kernel under allow-all rules, and of beam_select_close_kernel under close=True, for k = 1, 3, 8"""
    assert guard.hits(np.full((1, 16), 5), 16, 16) == [[]] and guard.banned([5] * 16, 16, 16) == {5}
    ref = _case(vocab, images=3, bias=LOOP)
    d = ref.d
    m = _model(ref, dtype, eos=d.eos)
    img = ref.img.cuda()
    g = (16, 16)
    crules = close_ref.closing_counter_rules(vocab, d.eos, 8, {d.bos, d.pad})
    for k in (1, 3, 8):
        plain = m.beam_search(img, k, 16, return_logp=True)
        assert m._engine.query(Q_LAST_GUARDED) == 0
        guarded = m.beam_search(img, k, 16, return_logp=True, repeat_guard=g)
        assert m._engine.query(Q_LAST_GUARDED) == 1 and guarded.rule_state is None
        _same(plain, guarded, tag=(k, "free"))
        ruled = m.beam_search(img, k, 16, return_logp=True, rules=_allow_all(vocab))
        _same(ruled, m.beam_search(img, k, 16, return_logp=True, rules=_allow_all(vocab), repeat_guard=g),
              ("tokens", "scores", "lengths", "logp", "rule_state"), (k, "allow-all"))
        _same(ruled, plain, tag=(k, "allow-all is plain"))
        closing = m.beam_search(img, k, 16, return_logp=True, rules=crules, close=True)
        _same(closing, m.beam_search(img, k, 16, return_logp=True, rules=crules, close=True, repeat_guard=g),
              ("tokens", "scores", "lengths", "logp", "rule_state"), (k, "closing"))


# ---- 3. every step is the float64 replay ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,vocab,dtype,g,lanes", [(1, 64, "fp32", (1, 1), 0), (4, 67, "fp32", (2, 1), 0), (8, 64, "fp32", (4, 2), 0),
                                                   (4, 1100, "fp32", (4, 2), 0), (8, 1100, "bf16", (2, 1), 0), (4, 64, "bf16", (1, 1), 0),
                                                   (1, 67, "bf16", (4, 2), 0), (4, 67, "fp32", (4, 2), 2)])
def test_every_step_is_the_float64_replay(k, vocab, dtype, g, lanes):
    """beam_ref.replay_pairs over ALL positions 0 .. STEPS - 1 with the float64 log-probabilities masked per beam by the guard on that beam's
    own prefix: ancestry, score increments, selection, order, ties.  k = 1, 4, 8; guards (1, 1), (2, 1), (4, 2); V = 64 / 67 (the register
    path's two request shapes) and 1100 (the general path); lanes = 2: two row ranges (slots and histories are range-local)"""
    ref = _case(vocab, bias=LOOP2 if g[0] >= 4 else LOOP)
    m = _model(ref, dtype)
    img = ref.img.cuda()
    free = m.beam_search(img, k, STEPS)
    assert _loops(free.tokens, *g) > 0, "the free search does not repeat: nothing would be tested"
    with knobs(TXO_LANES=lanes) if lanes else knobs():
        states, beams = _states(m, img, k, range(1, STEPS + 1), return_logp=True, repeat_guard=g)
        if lanes:
            assert m._engine.query(Q_LAST_ROW_RANGES) == lanes
    assert sorted(states) == list(range(1, STEPS + 1))
    periods = set()
    rep = br.replay_pairs(ref.s64, ref.enc64, ref.d.bos, None, states, range(STEPS), _eps_bf16 if dtype == "bf16" else _eps_fp32,
                          logp_of=_guarded_logp_of(ref, g, periods=periods))
    print(f"\nguarded beam replay k = {k}, V = {vocab}, {dtype}, guard {g}, ranges {lanes or 1}: {rep.steps} steps, max |score increment - "
          f"float64 log-prob| {rep.inc_err:.3e}, smallest selection slack {rep.slack:.3e} (float64's own margin {rep.gap:.1e}), ties {rep.ties}, "
          f"periods in force {sorted(periods)}")
    assert rep.steps == STEPS
    last = beams[STEPS]
    assert not torch.equal(last.tokens, free.tokens), "the guard never moved the search: nothing was tested"
    assert len(periods) >= min(2, g[0]), periods                   # bans of two different periods were in force (one, where P = 1)
    tok, sc = last.tokens.cpu().numpy(), last.scores.cpu().numpy()
    assert np.isfinite(sc).all()
    for b in range(tok.shape[0]):
        for r in range(k):
            assert guard_ref.violations(tok[b, r].tolist(), *g) == [], (b, r, tok[b, r].tolist())
    acc = torch.zeros_like(last.scores)                            # the increments summed left to right in float32 are the score, bit for bit
    for t in range(STEPS):
        acc = acc + last.logp[:, :, t]
    assert torch.equal(acc, last.scores)


# ---- 4. rules and the yield rule --------------------------------------------------------------------------------------------------------------
def _only(vocab, allowed):
    """one state; exactly `allowed` may be picked (eos is not among them)"""
    return R.TokenRules(R.pack(flags=np.where(np.isin(np.arange(vocab), allowed), 0, R.BAN))[None], 1).validate(vocab)


@pytest.mark.parametrize("vocab", [64, 1100])
def test_one_allowed_token_the_ban_is_dropped_at_every_pick(vocab):
    """rules that allow exactly one token, guard (1, 1): from position 1 on the guard bans that token, nothing is allowed and unbanned, and
    the ban is dropped -- the rules-only search, bit for bit, dead slots included"""
    ref = _case(vocab, bias=LOOP)
    m = _model(ref)
    img = ref.img.cuda()
    rules = _only(vocab, (9,))
    for k in (1, 4):
        want = m.beam_search(img, k, STEPS, return_logp=True, rules=rules)
        got = m.beam_search(img, k, STEPS, return_logp=True, rules=rules, repeat_guard=(1, 1))
        _same(want, got, ("tokens", "scores", "lengths", "logp", "rule_state"), k)
        assert bool((got.tokens[:, 0] == 9).all()) and bool(torch.isfinite(got.scores[:, 0]).all())
        assert got.tokens.shape[2] == STEPS and _loops(got.tokens[:, :1], 1, 1) == 2


@pytest.mark.parametrize("k,vocab,dtype", [(4, 64, "fp32"), (2, 1100, "fp32"), (4, 67, "bf16")])
def test_two_allowed_tokens_replayed_with_the_yield_rule(k, vocab, dtype):
    """rules that allow two tokens, guard (2, 1): behind a b a both are banned (periods 1 and 2) and the ban is dropped; every step is the
    float64 replay with beam_guard_ref.keep's mask, yields included; rule_state is rules.run's for every live beam"""
    ref = _case(vocab, bias=LOOP)
    m = _model(ref, dtype)
    img = ref.img.cuda()
    rules, g = _only(vocab, (5, 9)), (2, 1)
    states, beams = _states(m, img, k, range(1, STEPS + 1), return_logp=True, rules=rules, repeat_guard=g)
    periods, yields = set(), set()
    rep = br.replay_pairs(ref.s64, ref.enc64, ref.d.bos, None, states, range(STEPS), _eps_bf16 if dtype == "bf16" else _eps_fp32,
                          logp_of=_guarded_logp_of(ref, g, rules=rules, periods=periods, yields=yields))
    assert rep.steps == STEPS and periods == {1, 2} and yields, (periods, yields)
    last = beams[STEPS]
    assert _check_live_beams(rules, last, None) >= 2
    assert not torch.equal(last.tokens, m.beam_search(img, k, STEPS, rules=rules).tokens)


# ---- 5. closing ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,vocab", [(3, 64), (5, 1100)])
def test_closing_search_keeps_its_guarantee_under_the_guard(k, vocab):
    """the counter rules with eos enabled, close=True, guard (2, 1), 12 positions: every live beam is finished, passes rules.run, has
    rules.run's state, and every token is either unbanned or stands where the closing-allowed set minus the ban set was empty"""
    N, g = 12, (2, 1)
    ref = _case(vocab, bias={(5,): 4.0, (6,): 3.5, (12,): 3.0})    # 5 opens, 6 closes, 12 is neutral: loops that move the depth
    d = ref.d
    m = _model(ref, eos=d.eos)
    img = ref.img.cuda()
    rules = close_ref.closing_counter_rules(vocab, d.eos, 8, {d.bos, d.pad})
    dist = rules.close_dist(d.eos)
    plain = m.beam_search(img, k, N, rules=rules, close=True, return_logp=True)
    got = m.beam_search(img, k, N, rules=rules, close=True, return_logp=True, repeat_guard=g)
    assert m._engine.query(Q_LAST_GUARDED) == 1
    assert _loops(plain.tokens, *g, eos=d.eos) > 0, "the closing search does not repeat: nothing would be tested"
    assert not torch.equal(plain.tokens, got.tokens)
    assert _check_live_beams(rules, got, d.eos) >= 2
    tok, sc, ln = (x.cpu().numpy() for x in (got.tokens, got.scores, got.lengths))
    held = 0
    for b in range(tok.shape[0]):
        for r in range(k):
            if not np.isfinite(sc[b, r]):
                continue
            row = tok[b, r, :ln[b, r]].tolist()
            assert ln[b, r] <= N and row[-1] == d.eos and d.eos not in row[:-1], (b, r, row)
            for i, t in enumerate(row):
                ban = guard_ref.banned(row[:i], *g, d.eos)
                held += bool(ban)
                if t in ban:
                    state = rules.run(row[:i])[0]
                    allowed = rules.allowed(state[None], remaining=N - i, ended=np.zeros(1, bool), dist=dist)[0]
                    allowed[sorted(ban)] = False
                    assert not allowed.any(), (b, r, i, row)
    assert held > 0


# ---- 6. ragged --------------------------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_equals_every_image_alone():
    """fp32, two sizes in one list, under the guard: beams, scores, lengths and logp of an image are its solo call's, bit for bit"""
    ref = _case(64, bias=LOOP)
    m = _model(ref)
    g = (4, 2)
    imgs = [rgb_images(1, h, w, 91 + i)[0].cuda() for i, (h, w) in enumerate([(48, 64), (32, 48)])]
    free = m.beam_search(imgs, 4, STEPS)
    got = m.beam_search(imgs, 4, STEPS, return_logp=True, repeat_guard=g)
    assert _loops(free.tokens, *g) > 0 and _loops(got.tokens, *g) == 0
    for b, im in enumerate(imgs):
        one = m.beam_search(im[None], 4, STEPS, return_logp=True, repeat_guard=g)
        for name in ("tokens", "scores", "lengths", "logp"):
            assert torch.equal(getattr(got, name)[b], getattr(one, name)[0]), (b, name)
        assert torch.equal(m.beam_search([im], 4, STEPS, return_logp=True, repeat_guard=g).tokens, one.tokens)


# ---- 7. generate(beam=k, repeat_guard=) -----------------------------------------------------------------------------------------------------------
def test_generate_beam_is_beam_searchs_best_beam():
    ref = _case(64, bias=LOOP)
    m = _model(ref)
    eng = m._engine
    img = ref.img.cuda()
    g = (2, 1)
    before = m.beam_search(img, 4, STEPS, return_logp=True)
    before3 = m.generate(img, STEPS, beam=4, return_beams=True)
    want = m.beam_search(img, 4, STEPS, repeat_guard=g)
    best = m.generate(img, STEPS, beam=4, repeat_guard=g)
    assert eng.query(Q_LAST_GUARDED) == 1 and eng.repeat_guard is None
    assert torch.equal(best, want.tokens[:, 0]) and not torch.equal(best, before.tokens[:, 0])
    toks, scores = m.generate(img, STEPS, beam=4, return_beams=True, repeat_guard=g)
    assert torch.equal(toks, want.tokens) and torch.equal(scores, want.scores)
    after3 = m.generate(img, STEPS, beam=4, return_beams=True)
    assert eng.query(Q_LAST_GUARDED) == 0
    assert torch.equal(after3[0], before3[0]) and torch.equal(after3[1], before3[1])
    _same(m.beam_search(img, 4, STEPS, return_logp=True), before)
    assert eng.query(Q_LAST_GUARDED) == 0
    m.generate(img, STEPS, repeat_guard=g)                        # the guarded generate sets it as ever
    assert eng.query(Q_LAST_GUARDED) == 1


def test_vocabulary_beyond_the_lds_is_refused_by_name():
    """50 000 entries, 8 beams, guard (16, 16): 8 * (271 * 4 + 1563 * 4) = 58 688 bytes of maps and windows pass the 56 KB the selection may
    take -- ValueError that names the vocabulary, behind every other refusal of the entry; the engine is usable after it: the same guard
    with 4 beams (29 344 bytes) runs on the general path and obeys the guard, and the plain search gives the bits it gave before"""
    from test_gpu_rules import _tiny
    d = _tiny(50000)
    sd = synth.synth_state_dict(d, 3)
    b = sd["decoder.net.to_logits.bias"].copy()
    b[[5, 9]] += 8.0
    sd["decoder.net.to_logits.bias"] = b
    _, _, m = build(d, sd=sd, max_batch=8)
    m.eos_token = None
    m.guard_beam = True
    img = rgb_images(1, 48, 64, 41).cuda()
    before = m.beam_search(img, 8, 6, return_logp=True)
    for call in (lambda: m.beam_search(img, 8, 6, repeat_guard=(16, 16)), lambda: m.generate(img, 6, beam=8, repeat_guard=(16, 16)),
                 lambda: m.beam_search([img[0]], 8, 6, repeat_guard=(16, 16))):
        with pytest.raises(ValueError, match=r"beam search: the vocabulary does not fit the guarded selection's LDS .*the vocabulary has 50000 entries"):
            call()
    with pytest.raises(ValueError, match=r"beams in \[1, 8\], got 9"):                   # the call's own refusals come first
        m.beam_search(img, 9, 6, repeat_guard=(16, 16))
    assert m._engine.repeat_guard is None
    got = m.beam_search(img, 4, 8, return_logp=True, repeat_guard=(16, 16))            # fits: 4 beams
    assert m._engine.query(Q_LAST_GUARDED) == 1 and bool(torch.isfinite(got.scores).all())
    small = m.beam_search(img, 8, 8, repeat_guard=(1, 1))                               # 8 * (1 * 4 + 6252) bytes: fits as well
    assert _loops(m.beam_search(img, 8, 8).tokens, 1, 1) > 0 and _loops(small.tokens, 1, 1) == 0
    _same(m.beam_search(img, 8, 6, return_logp=True), before)


# ---- 8. the C example and the wrapper ---------------------------------------------------------------------------------------------------------------
def test_torch_free_c_program(tmp_path):
    """examples/beam_guard_tiny.c: plain C + the HIP runtime API: the refusal with the switch off, a free search that loops, the guarded
    beams (printed: none of them holds a token guard_ref bans), and the free beams again behind the guard"""
    import re
    import subprocess
    import sys
    from texocr_amd import build as b
    exe = b.build_example(verbose=False, name="beam_guard_tiny")
    blob = str(tmp_path / "tiny.bin")
    subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), "examples", "make_tiny_blob.py"), blob], check=True, capture_output=True)
    r = subprocess.run([exe, blob], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "switch off: beam search: not available while a repeat guard is set" in r.stdout
    assert "are the first run's" in r.stdout
    P, Rr, eos = (int(x) for x in re.search(r"guard \((\d+), (\d+)\), eos (-?\d+)", r.stdout).groups())
    eos = None if eos < 0 else eos
    free = [[int(t) for t in row.split()] for row in re.findall(r"^free beam \d+ \d+:((?: \d+)+)$", r.stdout, re.M)]
    rows = [[int(t) for t in row.split()] for row in re.findall(r"^guarded beam \d+ \d+:((?: \d+)+)$", r.stdout, re.M)]
    assert len(rows) == len(free) >= 4
    assert any(guard_ref.violations(_cut(row, eos), P, Rr, eos) for row in free), "the free beams do not repeat: nothing was tested"
    for row in rows:
        assert guard_ref.violations(_cut(row, eos), P, Rr, eos) == [], row


def test_wrapper_guarded_beam(tmp_path):
    """TeXOCRWrapper(cfg, guard_beam=True, repeat_guard=(1, 1)) with decode='beam': the batch equals the per-image calls, no row holds a
    violation, and repeat_guard=False on a call loops again"""
    from PIL import Image
    from texocr_amd.config import default_config
    from texocr_amd.wrapper import TeXOCRWrapper
    v = json.load(open(os.path.join(HERE, "golden", "tokenizer_vocab_1k.json")))
    tk = RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"])
    tk.save(str(tmp_path / "vocab.txt"))
    cfg = default_config(img_size=[64, 256], max_length=32, in_channels=1,
                         encoder={"embed_dim": 64, "heads": 2, "num_layers": 1}, decoder={"embed_dim": 64, "heads": 2, "num_layers": 2})
    cfg["tokenizer_path"] = str(tmp_path / "vocab.txt")
    with pytest.raises(ValueError, match="repeat_guard is not available with decode='beam'"):
        TeXOCRWrapper(cfg, max_batch=9, repeat_guard=(1, 1))(Image.new("RGB", (40, 30), "white"), max_len=8, decode="beam", beams=3)
    w = TeXOCRWrapper(cfg, max_batch=9, guard_beam=True, repeat_guard=(1, 1))
    assert w.model.guard_beam is True
    sd = synth.synth_state_dict(w.dims, 5)
    b = sd["decoder.net.to_logits.bias"].copy()
    b[[40, 41, 42]] += 4.0                                        # a few favoured tokens: the free beams loop
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
    assert [g[0] for g in got] == [o[0] for o in one]
    for g in got:
        assert guard_ref.violations(g[0], 1, 1, eos) == [], g[0]
    free = w.batch(pil, max_len=20, decode="beam", beams=3, repeat_guard=False)
    assert any(guard_ref.violations(f[0], 1, 1, eos) for f in free), "the free beams do not repeat: nothing was tested"
    assert w.model._engine.repeat_guard is None
