"""The beam selection under the repeat guard (csrc/beam_guard.h) at long periods and long windows, on tests/guard_zoo.py's scripted decoders.

tests/test_gpu_beam_guard.py puts bans of period 1, 2 and 4 in force over 14 positions: the staged window never passes 11 tokens, the
staging loop never goes round twice, and no more than 32 threads scan.  Here the script loops with period 5, 8 and 16, so the windows are
19 to 271 tokens, up to 128 (parent, period) threads scan, and k * L passes 256.  Nothing is restated: every step is tests/beam_ref.py's
float64 replay with tests/test_gpu_beam_guard.py's guarded mask (tests/beam_guard_ref.keep on tests/guard_ref.py's brute force) and the
eps imported from tests/test_gpu_beam.py.

Of the guards the replay runs under, (8, 2), (16, 1) and (5, 3) have windows of 23, 31 and 19 tokens: with at most 8 beams they stage at
most 248 entries, so `k * min(t, W) > 256` is asserted where the guard admits it -- (16, 2) at k = 8 (376, every step replayed) and
(16, 16) (271 per beam) -- and printed for every case."""
import numpy as np
import pytest
import torch

import beam_ref as br
import close_ref
import guard_ref
import guard_zoo as gz
from gpu_harness import knobs, rgb_images
from test_gpu_beam import _Ref, _eps_bf16, _eps_fp32
from test_gpu_beam_guard import _guarded_logp_of, _loops, _model, _only, _states
from test_gpu_beam_rules import _check_live_beams, _cut
from texocr_amd import guard
from texocr_amd._lib import Q_LAST_GUARDED, Q_LAST_ROW_RANGES

pytestmark = pytest.mark.gpu

_REFS = {}


def _ref(period, vocab, images=1, table=64, at=None):
    key = (period, vocab, images, table, tuple(sorted((at or {}).items())))
    if key not in _REFS:
        L = gz.loop(period, vocab)
        d = gz.dims(vocab, table)
        script = gz.loop_script(L.block, L.escapes, table, at={t: list(r) for t, r in (at or {}).items()})
        _REFS[key] = (_Ref(d, gz.scripted_sd(d, script), rgb_images(images, 48, 64, 40 + images)), script)
    return _REFS[key]


def _moved(rep):
    """steps of a replay at which a beam continues another slot than its own"""
    return sum(bool((p != np.arange(p.shape[1])[None]).any()) for p in rep.parents.values())


def _sum_is_score(res):
    acc = torch.zeros_like(res.scores)                             # the increments summed left to right in float32 are the score, bit for bit
    for t in range(res.logp.shape[2]):
        acc = acc + res.logp[:, :, t]
    return torch.equal(acc, res.scores)


# ---- 1. every step is the float64 replay, at long periods ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k,vocab,dtype,g,period,n,lanes", [(4, 64, "fp32", (8, 2), 8, 40, 0), (8, 67, "fp32", (16, 1), 16, 44, 0),
                                                          (4, 1100, "fp32", (5, 3), 5, 40, 0), (8, 1100, "bf16", (8, 2), 8, 40, 0),
                                                          (8, 64, "fp32", (16, 2), 16, 56, 0), (4, 67, "fp32", (5, 3), 5, 40, 2)])
def test_every_step_is_the_float64_replay_at_long_periods(k, vocab, dtype, g, period, n, lanes):
    """guards (8, 2), (16, 1), (5, 3), (16, 2) over 40 to 56 positions, k = 4 and 8, V = 64 / 67 (register path) and 1100 (general path),
    one case on two row ranges: every step replayed; a ban of the script's period (>= 5) is in force; some beam continues another slot
    than its own (the window is read through path_cur along an ancestry that moved); the staged k * L is printed, and passes 256 where
    the guard admits it"""
    ref, script = _ref(period, vocab, images=2 if lanes else 1)
    m = _model(ref, dtype, beams=k)
    img = ref.img.cuda()
    free = m.beam_search(img, k, n)
    assert _loops(free.tokens, *g) > 0, "the free search does not repeat: nothing would be tested"
    with knobs(TXO_LANES=lanes) if lanes else knobs():
        states, beams = _states(m, img, k, range(1, n + 1), return_logp=True, repeat_guard=g)
        if lanes:
            assert m._engine.query(Q_LAST_ROW_RANGES) == lanes
    assert sorted(states) == list(range(1, n + 1))
    periods = set()
    rep = br.replay_pairs(ref.s64, ref.enc64, ref.d.bos, None, states, range(n), _eps_bf16 if dtype == "bf16" else _eps_fp32,
                          logp_of=_guarded_logp_of(ref, g, periods=periods))
    W = gz.window(*g)
    staged, moved = k * min(n - 1, W), _moved(rep)
    print(f"\n[guard] beam replay k = {k}, V = {vocab}, {dtype}, guard {g}, script period {period}, ranges {lanes or 1}: {rep.steps} steps, "
          f"periods in force {sorted(periods)}, longest binding scan {max(g[1] * p - 1 for p in periods)}, window {W}, largest staged k*L "
          f"{staged}, {k * g[0]} scanning threads, steps with a moved ancestry {moved}, max |increment - float64| {rep.inc_err:.3e}, "
          f"smallest slack {rep.slack:.3e}")
    assert rep.steps == n
    assert period in periods and max(periods) >= 5, periods
    assert moved > 0
    assert n - 1 > W                                               # L = min(t, W) with t > W
    if g == (16, 2):
        assert staged > 256 and k * g[0] > 32
    last = beams[n]
    assert not torch.equal(last.tokens, free.tokens)
    tok = last.tokens.cpu().numpy()
    assert np.isfinite(last.scores.cpu().numpy()).all()
    for b in range(tok.shape[0]):
        for r in range(k):
            assert guard_ref.violations(tok[b, r].tolist(), *g) == [], (b, r)
    assert _sum_is_score(last)


# ---- 2. the longest window -------------------------------------------------------------------------------------------------------------
def test_window_of_271_tokens():
    """guard (16, 16) over 280 positions on the period-16 script: W = 271.  The first ban binds at position 271, behind 255 comparisons; the
    steps 269 .. 273 around it are replayed in float64 at k = 8 (a full replay would be 280 decodes).  k = 1 is the guarded greedy
    generate(), token for token (the script's margins are far above float32 rounding of logit - lse: tests/test_guard_zoo_cpu.py).  For
    every k: no beam holds a token the guard bans, scores are finite and the float32 sum of the logp increments, bit for bit"""
    g, n, period = (16, 16), 280, 16
    ref, script = _ref(period, 64, table=gz.TABLE)
    m = _model(ref, beams=8)
    img = ref.img.cuda()
    W = gz.window(*g)
    greedy = m.generate(img, n, repeat_guard=g)
    assert guard.hits(greedy.cpu().numpy(), *g)[0][0] == 271
    for k in (1, 4, 8):
        res = m.beam_search(img, k, n, return_logp=True, repeat_guard=g)
        assert m._engine.query(Q_LAST_GUARDED) == 1
        tok = res.tokens.cpu().numpy()
        assert np.isfinite(res.scores.cpu().numpy()).all() and _sum_is_score(res)
        assert guard.violations(tok[0], *g) == [[]] * k
        assert guard_ref.violations(tok[0, 0].tolist(), *g) == []
        if k == 1:
            assert torch.equal(res.tokens[:, 0], greedy)
        assert k * min(n - 1, W) > 256
        free = m.beam_search(img, k, n)
        assert _loops(free.tokens[:, :1], *g) > 0 and not torch.equal(free.tokens, res.tokens)
    around = range(269, 274)
    states, _ = _states(m, img, 8, range(around[0], around[-1] + 2), repeat_guard=g)
    periods = set()
    rep = br.replay_pairs(ref.s64, ref.enc64, ref.d.bos, None, states, around, _eps_fp32, logp_of=_guarded_logp_of(ref, g, periods=periods))
    assert rep.steps == len(around) and periods == {16}, periods
    print(f"\n[guard] beam window (16, 16): window {W}, largest staged k*L {8 * W}, longest binding scan 255, periods in force {sorted(periods)}, "
          f"{rep.steps} steps replayed around position 271, smallest slack {rep.slack:.3e}")


# ---- 3. beside rules, and a closing search -------------------------------------------------------------------------------------------------
def test_beside_token_rules():
    """period-8 script, guard (8, 2), rules that allow the block and two escapes only: every step is the replay with the yield rule, and
    rule_state is rules.run's"""
    k, n, g = 4, 30, (8, 2)
    ref, script = _ref(8, 64)
    L = gz.loop(8, 64)
    rules = _only(64, L.block + L.escapes[:2])
    m = _model(ref, beams=k)
    img = ref.img.cuda()
    states, beams = _states(m, img, k, range(1, n + 1), return_logp=True, rules=rules, repeat_guard=g)
    periods, yields = set(), set()
    rep = br.replay_pairs(ref.s64, ref.enc64, ref.d.bos, None, states, range(n), _eps_fp32,
                          logp_of=_guarded_logp_of(ref, g, rules=rules, periods=periods, yields=yields))
    assert rep.steps == n and 8 in periods, periods
    last = beams[n]
    assert _check_live_beams(rules, last, None) >= 2
    assert not torch.equal(last.tokens, m.beam_search(img, k, n, rules=rules).tokens)
    print(f"\n[guard] beam beside rules (8, 2): periods in force {sorted(periods)}, yields {len(yields)}")


def test_closing_search_at_period_8():
    """the counter rules with eos enabled, close=True, guard (8, 2), 30 positions on the period-8 script: every live beam is finished,
    passes rules.run with rules.run's state, and every token is unbanned or stands where the closing-allowed set minus the ban set was
    empty.  (A beam that ends early pays for eos once and never for an escape, so the guarded survivors are early finishers: that the guard
    bound is shown by the result differing from the plain closing search, which loops.)"""
    k, N, g = 4, 30, (8, 2)
    ref, script = _ref(8, 64)
    d = ref.d
    m = _model(ref, beams=k, eos=d.eos)
    img = ref.img.cuda()
    rules = close_ref.closing_counter_rules(64, d.eos, 8, {d.bos, d.pad})
    dist = rules.close_dist(d.eos)
    plain = m.beam_search(img, k, N, rules=rules, close=True, return_logp=True)
    got = m.beam_search(img, k, N, rules=rules, close=True, return_logp=True, repeat_guard=g)
    assert m._engine.query(Q_LAST_GUARDED) == 1
    assert _loops(plain.tokens, *g, eos=d.eos) > 0, "the closing search does not repeat: nothing would be tested"
    assert not torch.equal(plain.tokens, got.tokens)
    assert _check_live_beams(rules, got, d.eos) >= 1
    tok, sc, ln = (x.cpu().numpy() for x in (got.tokens, got.scores, got.lengths))
    for r in range(k):
        if not np.isfinite(sc[0, r]):
            continue
        row = tok[0, r, :ln[0, r]].tolist()
        assert ln[0, r] <= N and row[-1] == d.eos and d.eos not in row[:-1], (r, row)
        for i, t in enumerate(row):
            ban = guard_ref.banned(row[:i], *g, d.eos)
            if t in ban:
                allowed = rules.allowed(rules.run(row[:i])[0][None], remaining=N - i, ended=np.zeros(1, bool), dist=dist)[0]
                allowed[sorted(ban)] = False
                assert not allowed.any(), (r, i, row)


# ---- 4. finished beams inside the window ---------------------------------------------------------------------------------------------------
def test_finished_beams_inside_the_window():
    """eos enabled and ranked second at position 0, k = 8, guard (8, 2), 40 positions on the period-8 script: the beam that takes eos
    finishes at position 0 near -4 and stays among the eight (at k = 4 it is crowded out before the first ban binds at position 23); the
    others loop on with bans of period 8 in force.  Every step is the float64 replay with eos (a finished parent offers eos at + 0,
    unmasked); finished and live beams stand side by side at every length from the window W = 23 on; the finished beam repeats eos at a
    score that never changes, and its run of eos is no ban -- guard_ref bans nothing behind it, though without the eos exemption the
    same rows would ban eos from the second one on"""
    k, n, g = 8, 40, (8, 2)
    L = gz.loop(8, 64)
    eos = gz.dims(64, 64).eos
    ref, script = _ref(8, 64, at={0: (L.block[0], eos) + L.escapes[:2]})
    m = _model(ref, beams=k, eos=eos)
    img = ref.img.cuda()
    W = gz.window(*g)
    states, beams = _states(m, img, k, range(1, n + 1), return_logp=True, repeat_guard=g)
    assert sorted(states) == list(range(1, n + 1))                # the search does not end early: live beams remain
    periods = set()
    rep = br.replay_pairs(ref.s64, ref.enc64, ref.d.bos, eos, states, range(n), _eps_fp32, logp_of=_guarded_logp_of(ref, g, eos=eos, periods=periods))
    assert rep.steps == n and 8 in periods, periods
    frozen = set()
    for length in range(1, n + 1):
        tok, sc = states[length]
        fin = [r for r in range(k) if eos in tok[0, r].tolist()]
        assert len(fin) == 1, (length, fin)                       # one finished beam, seven live ones: side by side, from length 1 through the window and beyond
        row = tok[0, fin[0]].tolist()
        assert row == [eos] * length                              # finished at position 0, eos ever since
        frozen.add(sc[0, fin[0]].tobytes())
        assert guard_ref.banned(row, *g, eos) == set()            # the run of eos is no ban ...
        assert length < 2 or guard_ref.banned(row, *g) == {eos}   # ... which only the exemption makes so
    assert len(frozen) == 1                                       # the same float32 score at every length
    assert n > W
    last = beams[n]
    tok = last.tokens.cpu().numpy()[0]
    for r in range(k):
        assert guard_ref.violations(_cut(tok[r].tolist(), eos), *g, eos) == [], r
    free = m.beam_search(img, k, n)
    assert _loops(free.tokens, *g, eos=eos) > 0 and not torch.equal(free.tokens, last.tokens)
    print(f"\n[guard] beam with a finished beam (8, 2): periods in force {sorted(periods)}, finished at position 0, {n} steps replayed, window {W}")


# ---- 5. several bans in one map word ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [64, 1030])
def test_ruler_in_the_beam_selection(vocab):
    """one ranking a > b > c > d > x at every position under (8, 1): the guarded beams run along the ruler sequence a b a c a b a d ..., so a
    parent's ban set holds up to four RANKED tokens, several of them in one 32-bit word of its map (V = 64: 0, 1, 31; V = 1030, the
    general path: 1025, 1026 and 0, 1).  Every step is the float64 replay: a ban lost from the map would be selected"""
    case = next(c for c in gz.RULERS if c.vocab == vocab)
    k, n, g = 4, 20, (8, 1)
    key = ("ruler", vocab)
    if key not in _REFS:
        d = gz.dims(vocab, 32, case.low_specials)
        _REFS[key] = _Ref(d, gz.scripted_sd(d, gz.const_script(case.letters + (case.x,), 32)), rgb_images(1, 48, 64, 41))
    ref = _REFS[key]
    m = _model(ref, beams=k)
    img = ref.img.cuda()
    states, beams = _states(m, img, k, range(1, n + 1), return_logp=True, repeat_guard=g)
    periods, sizes = set(), []

    def logp_of(tokens, inner=_guarded_logp_of(ref, g, periods=periods)):
        for row in np.asarray(tokens)[0]:
            ban = guard_ref.banned(row.tolist(), *g)
            sizes.append((len(ban), gz.share_word(ban)))
        return inner(tokens)
    rep = br.replay_pairs(ref.s64, ref.enc64, ref.d.bos, None, states, range(n), _eps_fp32, logp_of=logp_of)
    assert rep.steps == n and {1, 2, 4, 8} <= periods, periods
    assert max(s for s, _ in sizes) >= 4 and any(w for s, w in sizes if s >= 3)          # four bans at once; three or more with two in one word
    print(f"\n[guard] beam ruler V = {vocab}: periods in force {sorted(periods)}, largest ban set {max(s for s, _ in sizes)}")
