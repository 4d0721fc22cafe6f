"""Repeat guard (include/texocr.h: txo_set_repeat_guard; csrc/step_guard.h) on the GPU.

The reference for every pick is a HOST REPLAY: tests/guard_ref.py (the rule by brute force) applied to the tokens before the pick and to
the logits the engine itself returned (return_logits=True holds the raw fp32 rows the selection read), so tokens are asserted exactly, in
fp32 and in bf16, with no tolerance: greedy = the arg-max of the masked row (lowest index on ties), sampled = tests/sampler_ref.py on the
masked row with tests/test_gpu_sampler.py's own treatment of draws next to a CDF boundary.  Where a path returns no logits (stop='row' with
compaction, captured steps, a prompted decode) a row is compared with the same guarded call on the simplest path, bit for bit in fp32.

The inputs were chosen on the CPU oracle (oracle/cpu_ref.py, 24 greedy positions): weight seed 5 with image seed 13 (vocabulary 64) and
image seed 11 (vocabulary 67) loop in every row under every guard used here; the tests assert that on the engine's own free decode."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import guard_ref
import sampler_ref as sr  # noqa: F401  (the sampler the draws are checked against, through test_gpu_sampler._check)
from gpu_harness import SHAPE_CASES, STOP_ENV, build, images, knobs, rgb_images, stop_case
from test_gpu_logp import FP32_LOGP, SAME_LOGITS
from test_gpu_sampler import _check as check_draws
from texocr_amd import guard
from texocr_amd import rules as R
from texocr_amd import synth
from texocr_amd._lib import Q_LAST_COMPACTIONS, Q_LAST_GUARDED, Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES
from texocr_amd.config import Dims

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = 24
GUARDS = [(1, 1), (4, 2), (16, 1), (3, 5)]
LOOP_IMAGES = {64: 13, 67: 11}                                    # vocabulary -> image seed (weight seed 5): see the module docstring


def _tiny(vocab, max_len=24):
    return Dims(canvas=64, in_channels=3, embed_dim=64, enc_heads=2, enc_layers=2, dec_heads=2, dec_layers=2, vocab=vocab,
                max_len=max_len, bos=vocab - 2, eos=vocab - 3, pad=vocab - 1)


def _loop_case(vocab, dtype="fp32", B=3, max_len=24, **kw):
    d, sd, m = build(_tiny(vocab, max_len), seed=5, dtype=dtype, max_batch=max(B, 4), **kw)
    m.eos_token = None
    return d, sd, m, rgb_images(B, 32, 48, LOOP_IMAGES[vocab]).cuda()


def replay_greedy(P, Rr, logits, tokens, eos=None, rules=None):
    """-> (the host's picks (B, n), bound (B, n): the RAW arg-max was banned, yields: picks at which the ban was dropped, final rule state),
    with the engine's tokens as the history"""
    logits, tokens = logits.float().cpu().numpy(), tokens.cpu().numpy()
    B, n, _ = logits.shape
    want, bound, yields = np.zeros((B, n), dtype=np.int64), np.zeros((B, n), dtype=bool), 0
    st = rules.start(B) if rules is not None else None
    for t in range(n):
        ok = rules.allowed(st) if rules is not None else [None] * B
        for b in range(B):
            row, ban, y = guard_ref.mask(logits[b, t], tokens[b, :t], P, Rr, eos, ok[b])
            want[b, t] = int(row.argmax())                        # (numpy's arg-max: the first maximum)
            bound[b, t] = int(logits[b, t].argmax()) in ban
            yields += int(y)
        if rules is not None:
            st, _ = rules.step(st, tokens[:, t])
    return want, bound, yields, st


def _gather64(logits, toks):
    return torch.log_softmax(logits.double().cpu(), -1).gather(2, toks.cpu()[..., None])[..., 0]


# ---- 1. every greedy pick against the replay -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,vocab", [("fp32", 64), ("fp32", 67), ("bf16", 64), ("bf16", 67)])
def test_every_greedy_pick_is_the_replay(dtype, vocab):
    """V % 4 == 0 (16-byte requests) and V % 4 != 0 (scalar stream); the four guards; no position is skipped"""
    d, sd, m, img = _loop_case(vocab, dtype)
    with knobs(TXO_PERSIST=0):
        free = m.generate(img, STEPS).cpu().numpy()
    for P, Rr in GUARDS:
        viol = guard.violations(free, P, Rr)
        # (1, 1) and (4, 2): every row of the free decode loops; (16, 1) and (3, 5): one row at least (in bf16 a row may escape a five-fold run)
        assert (all if (P, Rr) in ((1, 1), (4, 2)) else any)(len(v) >= 1 for v in viol), f"({P}, {Rr}): the free decode does not loop: the case is vacuous {viol}"
        toks, logits = m.generate(img, STEPS, return_logits=True, repeat_guard=(P, Rr))
        assert m._engine.query(Q_LAST_PERSISTENT) == 0 and m._engine.query(Q_LAST_GUARDED) == 1
        assert toks.shape == (3, STEPS) and logits.shape == (3, STEPS, vocab)
        want, bound, yields, _ = replay_greedy(P, Rr, logits, toks)
        assert np.array_equal(toks.cpu().numpy(), want), (P, Rr)
        assert bool(bound.any()), f"({P}, {Rr}): the raw arg-max was never banned"
        assert yields == 0
        assert guard.violations(toks.cpu().numpy(), P, Rr) == [[], [], []]
        assert [guard_ref.violations(r, P, Rr) for r in toks.cpu().tolist()] == [[], [], []]
        print(f"\n[guard] {dtype} V={vocab} ({P}, {Rr}): free violations {[len(v) for v in viol]}, the guard decided {int(bound.sum())} of {3 * STEPS} picks")
    assert m._engine.repeat_guard is None                         # the call's guard is gone behind it
    m.generate(img, STEPS)
    assert m._engine.query(Q_LAST_GUARDED) == 0


def test_the_reference_fixture_loops_and_the_guard_stops_it():
    """tests/golden/tiny.npz (the fixture test_guard_cpu.py counts on the host): the engine's free decode is the fixture's tokens, which loop
    in both rows under (1, 1) and (4, 2); guarded, every pick is the replay and no row violates"""
    meta = json.load(open(os.path.join(HERE, "golden", "tiny.json")))
    g = np.load(os.path.join(HERE, "golden", "tiny.npz"))
    d, sd, m = build(meta, max_batch=2)
    m.eos_token = None
    img = images(meta).cuda()
    n = g["tokens"].shape[1]
    assert np.array_equal(m.generate(img, n).cpu().numpy(), g["tokens"])
    for P, Rr in [(1, 1), (4, 2)]:
        assert all(len(v) >= 1 for v in guard.violations(g["tokens"], P, Rr))
        toks, logits = m.generate(img, n, return_logits=True, repeat_guard=(P, Rr))
        want, bound, _, _ = replay_greedy(P, Rr, logits, toks)
        assert np.array_equal(toks.cpu().numpy(), want) and bool(bound.any(1).all())
        assert guard.violations(toks.cpu().numpy(), P, Rr) == [[], []]


# ---- 2. sampled ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab,temp,seed,grd", [(1000, 0.3, 7, (1, 1)), (1030, 0.3, 11, (4, 1)), (67, 0.7, 2 ** 32 + 5, (16, 1)), (1000, 1.0, 3, (2, 1))])
def test_every_draw_on_the_masked_row(vocab, temp, seed, grd):
    """the register sampler with 16-byte loads (1000), the LDS sampler (1030, beyond the register limit), one-logit loads (67): every draw is
    sampler_ref's on the row with -3.4e38f where the guard bans.  Guards with max_repeats 1: the last token is banned at every pick behind
    the first, so every row but a row's first is a masked one (sampled rows of random weights rarely loop on their own)"""
    B, (P, Rr) = 4, grd
    d, sd, m = build(_tiny(vocab), seed=5, max_batch=B)
    m.eos_token = None
    img = rgb_images(B, 32, 48, 50).cuda()
    toks, logits = m.generate(img, STEPS, temp=temp, decode="sample", seed=seed, return_logits=True, repeat_guard=grd)
    assert m._engine.query(Q_LAST_PERSISTENT) == 0 and m._engine.query(Q_LAST_GUARDED) == 1
    tk, lg = toks.cpu().numpy(), logits.float().cpu().numpy()
    masked = np.empty_like(lg)
    n_ban = 0
    for b in range(B):
        for t in range(STEPS):
            masked[b, t], ban, y = guard_ref.mask(lg[b, t], tk[b, :t], P, Rr)
            n_ban += bool(ban)
            assert not y
    assert n_ban == B * (STEPS - 1), "a position behind the first had no ban"
    check_draws(f"guard V={vocab} {grd}", tk, masked.reshape(-1, vocab), temp, seed, np.repeat(np.arange(B), STEPS), np.tile(np.arange(STEPS), B))
    assert guard.violations(tk, P, Rr) == [[]] * B
    print(f"\n[guard] sampled V={vocab} {grd}: {n_ban} of {B * STEPS} positions had a ban")


# ---- 3. logp ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decode", ["greedy", "sample"])
@pytest.mark.parametrize("vocab", [64, 67])
def test_logp_is_the_raw_log_softmax(vocab, decode):
    """logp is log_softmax of the RAW returned logits at the committed token (test_gpu_logp's SAME_LOGITS) and what score() reports for the
    same tokens (its 2 * FP32_LOGP): a pick the guard forced keeps its low probability"""
    d, sd, m, img = _loop_case(vocab)
    toks, logits, logp = m.generate(img, STEPS, return_logits=True, return_logp=True, decode=decode, temp=0.3, seed=5, repeat_guard=(1, 1))
    assert float(logits.abs().max()) < 16                         # the premise of SAME_LOGITS
    e = float((logp.cpu().double() - _gather64(logits, toks)).abs().max())
    print(f"\n[guard] logp vs raw log_softmax V={vocab} {decode}: max |d| {e:.3e}")
    assert e < SAME_LOGITS, e
    if decode == "greedy":
        assert not torch.equal(toks, logits.argmax(-1))           # the guard moved picks off the raw arg-max: their logp is not the maximum's
    trg = torch.cat([torch.full((3, 1), d.bos, dtype=torch.int64, device="cuda"), toks], 1)
    s = m.score(img, trg, mask=torch.ones_like(trg, dtype=torch.bool))
    e2 = float((s.logp - logp).abs().max())
    print(f"[guard] logp vs score(): max |d| {e2:.3e}")
    assert e2 < 2 * FP32_LOGP, e2
    toks2, logp2 = m.generate(img, STEPS, return_logp=True, decode=decode, temp=0.3, seed=5, repeat_guard=(1, 1))      # without logits_out
    assert torch.equal(toks2, toks) and torch.equal(logp2, logp)


# ---- 4. guard off is today's decode ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [64, 67])
def test_guard_off_is_the_plain_launch_path(vocab):
    """repeat_guard=None, and a guard that can never bind on the decoded length ((16, 16) needs 17 copies of a block: 17 tokens at least,
    12 are decoded), give the tokens, logits and logp of the plain launch path bit for bit -- greedy and sampled"""
    d, sd, m, img = _loop_case(vocab)
    n = 12
    with knobs(TXO_PERSIST=0):
        plain = m.generate(img, n, return_logits=True, return_logp=True)
        none = m.generate(img, n, return_logits=True, return_logp=True, repeat_guard=None)
        assert m._engine.query(Q_LAST_GUARDED) == 0
        s_plain = m.generate(img, n, return_logits=True, return_logp=True, decode="sample", temp=1.0, seed=9)
    idle = m.generate(img, n, return_logits=True, return_logp=True, repeat_guard=(16, 16))
    assert m._engine.query(Q_LAST_GUARDED) == 1 and m._engine.query(Q_LAST_PERSISTENT) == 0
    s_idle = m.generate(img, n, return_logits=True, return_logp=True, decode="sample", temp=1.0, seed=9, repeat_guard=(16, 16))
    for name, a, b in (("None", plain, none), ("(16, 16)", plain, idle), ("(16, 16) sampled", s_plain, s_idle)):
        for x, y, what in zip(a, b, ("tokens", "logits", "logp")):
            assert torch.equal(x, y), (name, what)
    assert guard.hits(plain[0].cpu().numpy(), 16, 16) == [[], [], []]      # the guard had nothing to ban


# ---- 5. the prefix boundary ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Rr", [2, 3])
def test_prefix_boundary(Rr):
    """guard (2, R) behind periodic prefixes.  A logit bias makes a > b > c > e the model's order at every position, so a row's pick is the
    first of them its history does not ban.  Row 0's prefix is (a b) x R: m_2 = 2R - 2 at its first pick, a is not banned and is picked;
    from there its run straddles the prefix and its picks.  Row 1's prefix is b (a b) x R: m_2 = 2R - 1 at its first pick, the run lies
    wholly in the prefix and a is banned.  With a third row that starts at BOS the shortest prefix is 1 and every forced token is
    committed inside the loop; without it the multi-position pass consumes the first 2R columns."""
    V = 64
    d = _tiny(V, max_len=32)
    sd = synth.synth_state_dict(d, 5)
    a, b, c, e = 10, 11, 12, 13
    bias = sd["decoder.net.to_logits.bias"].copy()
    bias[[a, b, c, e]] += np.array([80.0, 60.0, 40.0, 20.0], dtype=bias.dtype)
    sd["decoder.net.to_logits.bias"] = bias
    _, _, m = build(d, sd=sd, max_batch=3)
    m.eos_token = None
    img = rgb_images(3, 32, 48, 95).cuda()
    n = 10
    rows = [[a, b] * Rr, [b] + [a, b] * Rr, []]
    width = 2 + 2 * Rr
    pre = torch.full((3, width), d.pad, dtype=torch.int64)
    for r, h in enumerate(rows):
        pre[r, 0] = d.bos
        pre[r, 1:1 + len(h)] = torch.tensor(h, dtype=torch.int64)
    lens = [1 + len(h) for h in rows]
    for B in (2, 3):
        toks, logp, plogp = m.generate(img[:B], n, prefix=pre[:B].cuda(), prefix_len=lens[:B], return_logp=True, repeat_guard=(2, Rr))
        assert m._engine.query(Q_LAST_GUARDED) == 1
        _, _, plogp0 = m.generate(img[:B], n, prefix=pre[:B].cuda(), prefix_len=lens[:B], return_logp=True)
        assert torch.equal(plogp, plogp0)                         # a forced token is never masked, and is scored as ever
        got = toks.cpu().tolist()
        for r in range(B):
            h = list(rows[r])
            for j in range(n):
                ban = guard_ref.banned(h, 2, Rr)
                want = next(x for x in (a, b, c, e) if x not in ban)
                assert got[r][j] == want, (B, r, j, h, got[r])
                h.append(want)
        assert got[0][0] == a and got[1][0] != a                  # the off-by-one pair at the boundary
        assert guard_ref.banned(rows[0], 2, Rr) == set() and guard_ref.banned(rows[1], 2, Rr) == {a}
        for r in range(B):                                        # single rows: the same call alone
            t1 = m.generate(img[r:r + 1], n, prefix=pre[r:r + 1, :lens[r]].cuda(), repeat_guard=(2, Rr))
            assert torch.equal(t1[0], toks[r]), (B, r)
    # sampled behind the prefix: a forced position consumes no draw; no row ends in R + 1 copies
    toks = m.generate(img, n, prefix=pre.cuda(), prefix_len=lens, decode="sample", temp=1.0, seed=4, repeat_guard=(2, Rr))
    for r in range(3):
        full = rows[r] + toks[r].cpu().tolist()
        assert [i for i in guard_ref.violations(full, 2, Rr) if i >= len(rows[r])] == [], r


# ---- 6. with rules ---------------------------------------------------------------------------------------------------------------------
def test_with_token_rules():
    """everything banned but {a, b, eos}, guard (2, 2): a token must be allowed AND unbanned, the replay runs guard_ref and the rules'
    numpy form together, rule_state is the host scan.  Then a rule set that allows ONE token (no eos): the guard yields at every pick it
    would ban that token, the row is all that token."""
    V = 64
    d, sd, m, img = _loop_case(V)
    a, b = 20, 33
    rules = R.ban(V, set(range(V)) - {a, b, d.eos})
    for decode in ("greedy", "sample"):
        toks, logits, state = m.generate(img, STEPS, return_logits=True, rules=rules, repeat_guard=(2, 2), decode=decode, temp=1.0, seed=6)
        assert m._engine.query(Q_LAST_GUARDED) == 1
        tk = toks.cpu().numpy()
        assert set(tk.reshape(-1).tolist()) <= {a, b, d.eos}
        st, ok = rules.run(tk[0])
        assert bool(ok.all())
        if decode == "greedy":
            want, bound, yields, st_all = replay_greedy(2, 2, logits, toks, rules=rules)
            assert np.array_equal(tk, want) and yields == 0
            assert np.array_equal(state.cpu().numpy(), st_all)
            free = m.generate(img, STEPS, rules=rules)[0].cpu().numpy()
            assert all(len(v) >= 1 for v in guard.violations(free, 2, 2)), "the constrained free decode never loops"
            assert not np.array_equal(tk, free)
        assert guard.violations(tk, 2, 2) == [[], [], []]
    one = R.ban(V, set(range(V)) - {a})
    for decode in ("greedy", "sample"):
        toks, logits, state = m.generate(img, STEPS, return_logits=True, rules=one, repeat_guard=(2, 2), decode=decode, temp=1.0, seed=6)
        assert bool((toks == a).all()), decode
        _, _, yields, st_all = replay_greedy(2, 2, logits, toks, rules=one)
        assert yields == 3 * (STEPS - 2)                          # from the third pick on (a a stands twice) the ban is dropped
        assert np.array_equal(state.cpu().numpy(), st_all)


# ---- 7. plumbing -----------------------------------------------------------------------------------------------------------------------
def test_row_stop_with_compactions_equals_every_image_alone():
    d, sd, img = stop_case()
    _, _, m = build(d, sd=sd, max_batch=40, env=STOP_ENV)
    img = img.cuda()
    with knobs(TXO_PERSIST=0):
        free = m.generate(img, 40, stop="row")
        toks = m.generate(img, 40, stop="row", repeat_guard=(1, 1))
    assert m._engine.query(Q_LAST_COMPACTIONS) >= 1 and m._engine.query(Q_LAST_GUARDED) == 1
    assert any(guard.violations(free.cpu().numpy(), 1, 1, eos=d.eos)), "the free decode never repeats a token"
    n = toks.shape[1]
    for r in range(0, 40, 3):
        t1 = m.generate(img[r:r + 1], 40, stop="row", repeat_guard=(1, 1))
        k = min(n, t1.shape[1])
        assert torch.equal(toks[r, :k], t1[0, :k]) and bool((toks[r, k:] == d.pad).all()), r
        row = toks[r].tolist()
        kept = row[:row.index(d.eos) + 1 if d.eos in row else n]
        assert guard_ref.violations(kept, 1, 1, d.eos) == [], r


def test_two_row_ranges():
    d, sd, m = build(_tiny(64), seed=5, max_batch=40)
    m.eos_token = None
    img = rgb_images(40, 32, 48, 81).cuda()
    with knobs(TXO_LANES=2):
        toks, logp = m.generate(img, 12, return_logp=True, repeat_guard=(4, 2))
        assert m._engine.query(Q_LAST_ROW_RANGES) == 2
    assert any(guard.hits(toks.cpu().numpy(), 4, 2))
    for r in (0, 19, 20, 39):
        t1, l1 = m.generate(img[r:r + 1], 12, return_logp=True, repeat_guard=(4, 2))
        assert torch.equal(toks[r], t1[0]) and torch.equal(logp[r], l1[0]), r


def test_captured_steps_ragged_window_and_from_enc():
    d, sd, m, img = _loop_case(64, max_len=8)
    grd = (2, 1)
    with knobs(TXO_GRAPH=1):
        tg, lg = m.generate(img, 8, return_logp=True, repeat_guard=grd)
        tg2 = m.generate(img, 8, repeat_guard=(1, 1))             # another guard on the same captured step: not the cached one
    with knobs(TXO_GRAPH=0):
        te, le = m.generate(img, 8, return_logp=True, repeat_guard=grd)
        te2 = m.generate(img, 8, repeat_guard=(1, 1))
    assert torch.equal(tg, te) and torch.equal(lg, le) and torch.equal(tg2, te2)
    assert guard.violations(te.cpu().numpy(), *grd) == [[], [], []] and any(guard.hits(te.cpu().numpy(), *grd))
    # the sliding window (beyond the 8-entry table; vocabulary a multiple of 8): the replay over the whole history, and every image alone
    tw, lw = m.generate(img, 13, return_logits=True, repeat_guard=grd)
    assert tw.shape == (3, 13)
    want, bound, _, _ = replay_greedy(*grd, lw, tw)
    assert np.array_equal(tw.cpu().numpy(), want) and bool(bound.any())
    for r in range(3):
        assert torch.equal(tw[r], m.generate(img[r:r + 1], 13, repeat_guard=grd)[0]), r
    # a ragged batch of three sizes
    imgs = [rgb_images(1, h, w, 91 + i)[0].cuda() for i, (h, w) in enumerate([(32, 64), (48, 48), (16, 32)])]
    tr, lr = m.generate_ragged(imgs, 8, return_logp=True, repeat_guard=grd)
    for r, im in enumerate(imgs):
        t1, l1 = m.generate(im[None], 8, return_logp=True, repeat_guard=grd)
        assert torch.equal(tr[r], t1[0]) and torch.equal(lr[r], l1[0]), r
    # from encoder rows
    enc = m.encoder(img)
    start = torch.full((3, 1), d.bos, dtype=torch.int64, device="cuda")
    assert torch.equal(m.decoder.generate(start, None, 8, enc=enc, repeat_guard=grd), te)
    with pytest.raises(ValueError, match="repeat_guard= needs the engine's own loop"):
        m.decoder.generate(start, None, 8, enc=enc, repeat_guard=grd, mask=torch.tensor([[False]] * 3))


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_and_scope():
    d, sd, m = build(dataclasses.replace(SHAPE_CASES["calib256"][0], vocab=1000, bos=998, eos=997, pad=999), seed=3, max_batch=4)
    eng = m._engine
    img = rgb_images(2, 64, 64, 99).cuda()
    plain = m.generate(img, 8)
    assert eng.query(Q_LAST_PERSISTENT) == 1
    for (P, Rr), text in [((0, 3), r"max_period is 0; it must be in \[1, 16\]"), ((17, 1), "max_period is 17"), ((2, 0), r"max_repeats is 0; it must be in \[1, 16\]"),
                          ((2, 17), "max_repeats is 17")]:
        with pytest.raises(ValueError, match="repeat guard: " + text):
            torch.ops.texocr.set_repeat_guard(eng.id, P, Rr)      # the engine's own refusal
        with pytest.raises(ValueError, match="repeat guard: " + text):
            m.generate(img, 8, repeat_guard=(P, Rr))              # ... and the host's, in the same words
        assert eng.repeat_guard is None
    brace = R.ban(1000, {5})
    with pytest.raises(ValueError, match="repeat guard: not available with a closing decode"):
        m.generate(img, 8, rules=brace, close=True, repeat_guard=(4, 3))
    assert eng.repeat_guard is None and eng.token_rules is None
    for call in (lambda: m.generate(img, 8, beam=2, repeat_guard=(4, 3)), lambda: m.beam_search(img, 2, 8, repeat_guard=(4, 3)),
                 lambda: m.beam_search([img[0], img[1, :, :32]], 2, 8, repeat_guard=(4, 3))):
        with pytest.raises(ValueError, match="beam search: not available while a repeat guard is set"):
            call()
        assert eng.repeat_guard is None
    assert m.beam_search(img, 2, 8).tokens.shape[:2] == (2, 2)    # ... and available again behind them
    # the engine is usable: a guarded call leaves the persistent launch, and the plain call is back on it with the same tokens
    toks = m.generate(img, 8, repeat_guard=(1, 1))
    assert eng.query(Q_LAST_PERSISTENT) == 0 and eng.query(Q_LAST_GUARDED) == 1 and guard.violations(toks.cpu().numpy(), 1, 1, d.eos) == [[], []]
    again = m.generate(img, 8)
    assert eng.query(Q_LAST_PERSISTENT) == 1 and eng.query(Q_LAST_GUARDED) == 0 and torch.equal(again, plain)
    # a guard set by hand stays across calls, and a call's repeat_guard= puts it back behind itself
    eng.set_repeat_guard((1, 1))
    assert torch.equal(eng.generate(img, 8, d.eos), toks)
    m.generate(img, 8, repeat_guard=(4, 2))
    assert eng.repeat_guard == (1, 1) and torch.equal(eng.generate(img, 8, d.eos), toks)
    eng.set_repeat_guard(None)
    assert eng.repeat_guard is None and torch.equal(m.generate(img, 8), plain)
    # V <= P + 1
    small = Dims(canvas=64, in_channels=3, embed_dim=64, enc_heads=2, enc_layers=1, dec_heads=2, dec_layers=1, vocab=8, max_len=8, bos=6, eos=5, pad=7)
    _, _, ms = build(small, seed=1, max_batch=1)
    with pytest.raises(ValueError, match=r"repeat guard: the vocabulary has 8 entries; it needs more than max_period \+ 1 = 8"):
        torch.ops.texocr.set_repeat_guard(ms._engine.id, 7, 1)
    with pytest.raises(ValueError, match=r"repeat guard: the vocabulary has 8 entries"):
        ms.generate(rgb_images(1, 32, 32, 1).cuda(), 4, repeat_guard=(7, 1))
    assert ms.generate(rgb_images(1, 32, 32, 1).cuda(), 4, repeat_guard=(6, 1)).shape == (1, 4)


# ---- 9. the C example and the wrapper --------------------------------------------------------------------------------------------------
def test_torch_free_c_program_under_a_guard(tmp_path):
    """examples/guard_tiny.c: plain C + the HIP runtime API: a free run, txo_set_repeat_guard(1, 1) and (4, 2), a refused guard, off again.
    The program prints its guarded rows; they satisfy guard_ref here."""
    import subprocess
    import sys
    from texocr_amd import build as b
    exe = b.build_example(verbose=False, name="guard_tiny")
    blob = str(tmp_path / "tiny.bin")
    subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), "examples", "make_tiny_blob.py"), blob], check=True, capture_output=True)
    r = subprocess.run([exe, blob], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "max_period is 17" in r.stdout and "are the first run's" in r.stdout
    import re
    rows = re.findall(r"^guard (\d+) (\d+) row \d+:((?: \d+)+)$", r.stdout, re.M)
    assert len(rows) >= 4 and {(int(P), int(Rr)) for P, Rr, _ in rows} == {(1, 1), (4, 2)}
    for P, Rr, toks in rows:
        assert guard_ref.violations([int(t) for t in toks.split()], int(P), int(Rr)) == [], (P, Rr, toks)


def test_wrapper_repeat_guard(tmp_path):
    """TeXOCRWrapper(..., repeat_guard=) / __call__ / batch(repeat_guard=): the batch equals the per-image calls, every returned row satisfies
    guard_ref, repeat_guard=False on a call switches it off again (and that run does loop)"""
    from PIL import Image
    from texocr_amd.config import default_config
    from texocr_amd.tokenizer import RegExTokenizer
    from texocr_amd.wrapper import TeXOCRWrapper
    v = json.load(open(os.path.join(HERE, "golden", "tokenizer_vocab_1k.json")))
    tk = RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"])
    tk.save(str(tmp_path / "vocab.txt"))
    cfg = default_config(img_size=[64, 256], max_length=32, in_channels=1,
                         encoder={"embed_dim": 64, "heads": 2, "num_layers": 1}, decoder={"embed_dim": 64, "heads": 2, "num_layers": 2})
    cfg["tokenizer_path"] = str(tmp_path / "vocab.txt")
    w = TeXOCRWrapper(cfg, max_batch=3, repeat_guard=(1, 1))
    sd = synth.synth_state_dict(w.dims, 5)
    bias = sd["decoder.net.to_logits.bias"].copy()
    bias[[100, 101, 102]] += 4.0                                  # three favoured tokens: the free run repeats them
    sd["decoder.net.to_logits.bias"] = bias
    w.model.load_state_dict(sd)
    rng = np.random.RandomState(0)
    pil = []
    for wd, ht in [(200, 40), (30, 30), (250, 64), (100, 17)]:
        arr = np.full((ht, wd, 3), 255, dtype=np.uint8)
        arr[rng.randint(0, ht, 40), rng.randint(0, wd, 40)] = rng.randint(0, 120, (40, 1))
        pil.append(Image.fromarray(arr))
    one = [w(im, max_len=20, decode="greedy") for im in pil]
    got = w.batch(pil, max_len=20, decode="greedy")
    free = w.batch(pil, max_len=20, decode="greedy", repeat_guard=False)
    eos = w.model.eos_token
    for x, y in zip(one, got):
        assert x[0] == y[0] and x[1] == y[1]
        assert guard_ref.violations(y[0], 1, 1, eos) == [], y[0]
    assert any(guard_ref.violations(f[0], 1, 1, eos) for f in free), "the free run never repeats a token: nothing was tested"
    assert w.model._engine.repeat_guard is None
    with pytest.raises(ValueError, match="repeat_guard is not available with decode='beam'"):
        w(pil[0], max_len=20, decode="beam")
    with pytest.raises(ValueError, match=r"repeat guard: max_period is 17"):
        TeXOCRWrapper(cfg, repeat_guard=(17, 1))
