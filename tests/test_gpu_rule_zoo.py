"""The token-rule kernels (csrc/step_rules.h, csrc/beam_rules.h) under rule sets whose states differ (tests/rule_zoo.py).

The method is tests/test_gpu_rules.py's, tests/test_gpu_rules_close.py's and tests/test_gpu_beam_rules.py's -- every pick replayed on the
host with no tolerance, through their own replays -- and nothing here restates the rule.  What is new is the rule sets: rows, deltas, clamps
and distance tables that differ by state, the full 8 x 256 distance table and one with a partial last 16-byte piece, and a state eos cannot
be reached from.  Every case carries guards -- asserted conditions on the run itself (the states visited, a clamp that happened, a pick the
budget moved in a state other than 0) -- without which a test would pass for a kernel that ignores what it is about."""
import numpy as np
import pytest
import torch

import beam_ref as br
import close_ref
import rule_zoo as zoo
import rules_ref
from gpu_harness import STOP_ENV, build, knobs, rgb_images, stop_case
from test_gpu_beam import _Ref
from test_gpu_beam_rules import _check_live_beams, _eps_fp32, _masked_logp_of, _states
from test_gpu_rules import _tiny, masked_rows, replay_greedy
from test_gpu_sampler import _check as check_draws
from texocr_amd import rules as R
from texocr_amd import synth
from texocr_amd._lib import Q_LAST_COMPACTIONS, Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES

pytestmark = pytest.mark.gpu

STEPS = 20
MAKE = {"skew": zoo.skew, "trap": zoo.trap, "wide": zoo.wide}
# logit offsets towards classes of STATE 0 (in another state the same ids belong to other classes): the opens that move the depth furthest,
# the closers with delta <= -2 (need = -delta, and the drop with need 0 that clamps), and eos
BIAS = {"skew": dict(open=2.0, deep=2.5, eos=1.0), "trap": dict(open=2.0, deep=2.5, eos=1.0), "wide": dict(open=2.5, deep=2.5, eos=1.0)}


def _np(x):
    return x.cpu().numpy()


def biased_sd(d, rules, seed, bias):
    need, delta, nxt, flags = R.unpack(rules.table[0])
    sd = synth.synth_state_dict(d, seed)
    b = sd["decoder.net.to_logits.bias"].copy()
    b[zoo.by_delta(rules, int(delta.max()))] += bias.get("open", 0.0)
    b[zoo.by_delta(rules, -2, lo=-128)] += bias.get("deep", 0.0)
    b[d.eos] += bias.get("eos", 0.0)
    sd["decoder.net.to_logits.bias"] = b
    return sd


def _case(name, vocab, dtype="fp32", seed=3, max_batch=5, max_len=24, bias=None, **kw):
    d = _tiny(vocab, max_len=max_len)
    rules = MAKE[name](vocab, d.eos, (d.bos, d.pad), **kw)
    sd = biased_sd(d, rules, seed, BIAS[name] if bias is None else bias)
    _, _, m = build(d, sd=sd, dtype=dtype, max_batch=max_batch)
    return d, sd, m, rules


def states_before(rules, tokens, state0=None):
    """(B, n, 2): the state every row stood in at every pick (rules.step over the row's own tokens)"""
    tokens = np.asarray(tokens)
    st = rules.start(tokens.shape[0]) if state0 is None else np.asarray(state0, dtype=np.int32)
    out = np.zeros(tokens.shape + (2,), dtype=np.int32)
    for t in range(tokens.shape[1]):
        out[:, t] = st
        st, _ = rules.step(st, tokens[:, t])
    return out


def _cut(rows, eos):
    return [row[:row.index(eos) + 1] if eos in row else row for row in np.asarray(rows).tolist()]


# (rule set, dtype, vocabulary, image seed): the seeds are those for which the float64 oracle's constrained decode meets every guard below
GREEDY = [("skew", "fp32", 64, 45), ("skew", "bf16", 67, 44), ("wide", "fp32", 1100, 46), ("wide", "fp32", 64, 44)]
CLOSING = [("skew", "fp32", 64, 44), ("skew", "bf16", 67, 44), ("wide", "fp32", 1100, 44), ("wide", "fp32", 64, 45), ("trap", "fp32", 64, 44),
           ("trap", "fp32", 67, 44)]


# ---- a. greedy, plain rules ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype,vocab,images", GREEDY)
def test_greedy_tokens_are_the_replay(name, dtype, vocab, images):
    """argmax_rules_step_kernel, rules_settle_kernel: tokens and rule_state are test_gpu_rules.replay_greedy's on the call's own logits"""
    B = 4
    d, sd, m, rules = _case(name, vocab, dtype)
    m.eos_token = None
    img = rgb_images(B, 48, 64, images).cuda()
    toks, logits, state = m.generate(img, STEPS, return_logits=True, rules=rules)
    assert m._engine.query(Q_LAST_PERSISTENT) == 0 and toks.shape == (B, STEPS)
    want, st, bound = replay_greedy(rules, logits, toks)
    ev = zoo.events(rules, _np(toks))
    print(f"\n[zoo] greedy {name} {dtype} V={vocab}: " + "; ".join(f"states {sorted(set(e.states))} deep {e.deep_close} clamp0 {e.clamp_zero} "
                                                                    f"need {e.max_need} depth {e.max_depth}" for e in ev))
    assert np.array_equal(_np(toks), want)
    assert np.array_equal(_np(state), st)
    assert bool(bound.any()), "no row met a disallowed arg-max: the test is vacuous"
    assert all(len(set(e.states)) >= 2 for e in ev), "a row stood in one state only: another state's row was never read"
    assert any(e.deep_close for e in ev), "no delta <= -2 was committed: the sign extension saw -1 / 0 / +1 only"
    assert any(e.clamp_zero for e in ev), "no commit clamped at depth 0"
    assert any(e.max_need >= 2 for e in ev), "no commit with need >= 2"
    assert not any(e.clamp_max for e in ev)                        # (only a forced token can)
    if name == "wide":
        assert any(e.max_depth >= 128 for e in ev), "no row reached depth 128: the upper half of the depth range was not used"


# ---- b. greedy, closing ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype,vocab,images", CLOSING)
def test_greedy_tokens_are_the_budgeted_replay(name, dtype, vocab, images):
    """argmax_rules_close_step_kernel (rules_close_start_kernel behind it): tokens = the arg-max of close_ref.replay's rows, the state is the
    replay's, every row ends at an allowed eos.  skew: dist depends on the state at every depth; wide: all 2048 nodes are staged; trap: a
    table with an unreachable state is budgeted at every position (slack = INT_MAX)."""
    B = 4
    d, sd, m, rules = _case(name, vocab, dtype)
    dist = rules.close_dist(d.eos)
    img = rgb_images(B, 48, 64, images).cuda()
    toks, logits, state = m.generate(img, STEPS, return_logits=True, rules=rules, close=True)
    assert m._engine.query(Q_LAST_PERSISTENT) == 0
    tk, lg = _np(toks), _np(logits.float())
    n = tk.shape[1]
    rows, st, ended = close_ref.replay(rules, dist, lg, tk, STEPS)
    plain, _, _ = close_ref.replay(rules, dist, lg, tk, STEPS, close=False)
    assert np.array_equal(tk, rows.argmax(2))
    assert np.array_equal(_np(state), st)
    assert bool(ended.all()) and all(close_ref.closed_rows(rules, tk, d.eos))
    before = states_before(rules, tk)
    open_yet = np.cumsum(tk == d.eos, 1) - (tk == d.eos) == 0      # the row had not committed an eos in front of this pick
    moved = (plain.argmax(2) != tk) & open_yet
    dd = np.asarray(dist)
    off0 = dd[before[..., 0], before[..., 1]] != dd[0, before[..., 1]]
    print(f"\n[zoo] closing greedy {name} {dtype} V={vocab}: {n} positions, the budget moved {int(moved.sum())} picks, "
          f"{int((moved & (before[..., 0] != 0)).sum())} of them in a state other than 0, {int((moved & off0).sum())} at a node whose distance is not state 0's")
    assert bool((moved & (before[..., 0] != 0)).any()), "the budget moved no pick in a state other than 0: the test is vacuous"
    assert bool((moved & off0).any()), "the budget moved no pick at a node whose distance differs from state 0's: the test is vacuous"
    if name == "trap":
        assert dist.any_inf
        slack = STEPS - np.arange(n) - 1 >= dist.dist_max          # positions at which a table without an infinite entry is not budgeted
        assert bool(((rows != plain).any(2) & open_yet)[:, slack].any()), "the budget masked nothing where R - 1 >= dist_max: the test is vacuous"
        assert all(2 not in zoo.events(rules, r)[0].states for r in _cut(tk, d.eos)), "a row entered the state eos cannot be reached from"
    if name == "wide":
        assert dd.size == 2048


# ---- c. sampled --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,vocab,temp,seed,close", [("skew", 1000, 1.0, 7, False), ("skew", 1000, 1.0, 7, True), ("skew", 67, 0.7, 2 ** 32 + 5, False),
                                                        ("skew", 67, 0.7, 2 ** 32 + 5, True), ("wide", 1030, 1.0, 12, True),
                                                        ("wide", 1030, 1.0, 12, False)])
def test_every_draw_on_the_masked_or_budgeted_row(name, vocab, temp, seed, close):
    """sample_rules_step_kernel / sample_rules_close_step_kernel, <true> with 16-byte loads (1000) and with one-logit loads (67), <false>
    (1030: the LDS sampler's dynamic LDS behind the static 4 KB table, all 2048 nodes staged): every draw is sampler_ref's on the row"""
    B = 5
    d, sd, m, rules = _case(name, vocab, seed=5)
    if not close:
        m.eos_token = None
    dist = rules.close_dist(d.eos)
    img = rgb_images(B, 48, 64, 50).cuda()
    toks, logits, state = m.generate(img, STEPS, temp=temp, decode="sample", seed=seed, return_logits=True, rules=rules, close=close)
    assert m._engine.query(Q_LAST_PERSISTENT) == 0
    tk = _np(toks)
    n = tk.shape[1]
    if close:
        rows, st, ended = close_ref.replay(rules, dist, _np(logits.float()), tk, STEPS)
        plain, _, _ = close_ref.replay(rules, dist, _np(logits.float()), tk, STEPS, close=False)
        assert bool((rows != plain).any()), "the budget masked nothing"
        assert bool(ended.all()) and all(close_ref.closed_rows(rules, tk, d.eos))
    else:
        rows, st = masked_rows(rules, logits, toks)
    check_draws(f"zoo {name} V={vocab} close={close}", tk, rows.reshape(-1, vocab), temp, seed, np.repeat(np.arange(B), n), np.tile(np.arange(n), B))
    assert np.array_equal(_np(state), st)
    ev = zoo.events(rules, tk)
    assert all(len(set(e.states)) >= 2 for e in ev), "a row stood in one state only: another state's row was never read"
    assert any(e.deep_close for e in ev), "no delta <= -2 was committed"
    before = states_before(rules, tk)
    a = rules.allowed(before.reshape(-1, 2)).reshape(B, n, vocab)
    assert bool((a != rules.allowed(np.stack([np.zeros(B * n, np.int32), before[..., 1].reshape(-1)], 1)).reshape(B, n, vocab)).any()), \
        "every mask equals state 0's at the same depth"


# ---- d. forced prefixes --------------------------------------------------------------------------------------------------------------------
def _path(rules, steps, state=(0, 0)):
    """token ids that take the automaton through `steps` = [(delta, next state), ...] from `state`: the lowest id of the current state's row
    with that delta and next (eos-like and banned entries apart)"""
    s, out = int(state[0]), []
    for delta, nx in steps:
        need, dl, nxt, flags = R.unpack(rules.table[s])
        ids = np.nonzero((dl == delta) & (nxt == nx) & (flags == 0))[0]
        assert ids.size, (s, delta, nx)
        out.append(int(ids[0]))
        s = nx
    return out


def _prompted(m, d, img, prefix, lens, n, **kw):
    pre = torch.full((len(prefix), max(lens)), 0, dtype=torch.int64)
    for r, row in enumerate(prefix):
        pre[r, :len(row)] = torch.tensor(row)
    return m.generate(img, n, prefix=pre.cuda(), prefix_len=lens, **kw)


def _teacher_logits(m, enc, d, prefix, toks):
    """a prompted decode keeps no logits: the engine's own teacher-forced logits of [prefix, picks] (decoder.net), the rows behind the prefix"""
    out = []
    for r, row in enumerate(prefix):
        full = torch.tensor([row + toks[r].tolist()[:-1]], dtype=torch.int64).cuda()
        out.append(m.decoder.net(full, enc=enc[r:r + 1])[0, len(row) - 1:].float().cpu().numpy())
    return np.stack(out)


def _assert_picks(rows, picks, where):
    """rows (B, V): the masked rows of teacher-forced logits, picks (B,): every pick is the row's arg-max; where the two best entries lie
    within the 1e-4 the fp32 logits of two kernels are held to, it is one of those two.  No pick goes unexamined."""
    order = np.argsort(rows, 1, kind="stable")
    for r in range(rows.shape[0]):
        a, b = int(order[r, -1]), int(order[r, -2])
        if rows[r, a] - rows[r, b] > 1e-4:
            assert int(picks[r]) == int(rows[r].argmax()), (where, r)
        else:
            assert int(picks[r]) in (a, b), (where, r, "a near-tie: neither of the two best")


SKEW_PATHS = ([(2, 0), (2, 0), (-3, 0), (-2, 0), (0, 1), (0, 2)], [(1, 1), (-1, 1)])
WIDE_PATHS = ([(127, 1), (127, 2), (-42, 3), (127, 4), (-128, 4), (0, 5), (0, 6), (0, 7), (0, 0), (-102, 0), (-102, 0)], [(1, 3), (-42, 2)])


@pytest.mark.parametrize("name,vocab,paths", [("skew", 64, SKEW_PATHS), ("wide", 1100, WIDE_PATHS)])
def test_forced_prefix_walks_every_state(name, vocab, paths):
    """rules_start_kernel (columns the multi-position pass consumed) and the forced commits of the step kernel (the longer row's further
    columns): two rows with prefixes of different lengths whose tokens pass through every state, hold a -3 / -128 token, a drop that clamps at
    0 and -- wide -- a +127 at depth 212 that the rules disallow, forced all the same, which clamps at 255.  The state returned is rules.run
    of prefix and picks, and every pick is the arg-max of the masked row of the engine's own teacher-forced logits (decoder.net; a prompted
    decode returns none) -- or, where that row's two best lie within 1e-4, one of those two (_assert_picks)."""
    d, sd, m, rules = _case(name, vocab, max_batch=2, max_len=32)
    m.eos_token = None
    img = rgb_images(2, 48, 64, 95).cuda()
    prefix = [[d.bos] + _path(rules, p) for p in paths]
    lens = [len(p) for p in prefix]
    ev = zoo.events(rules, prefix[0][1:])[0]
    assert set(ev.states) == set(range(rules.n_states)) and ev.deep_close and ev.clamp_zero and ev.max_need >= 3, "the prefix misses an event"
    if name == "wide":
        assert ev.clamp_max and ev.max_need == 128 and not bool(rules.run(prefix[0][1:])[1].all()), "no forced token clamps at depth_max"
    n = 8
    toks, state = _prompted(m, d, img, prefix, lens, n, rules=rules)
    assert m._engine.query(Q_LAST_PERSISTENT) == 0 and toks.shape == (2, n)
    start = np.stack([rules.run(p[1:])[0] for p in prefix])
    assert len({tuple(s) for s in start.tolist()}) == 2
    for r in range(2):
        st, ok = rules.run(prefix[r][1:] + toks[r].tolist())
        assert state[r].tolist() == st.tolist(), (r, state[r].tolist(), st.tolist())
        assert bool(ok[lens[r] - 1:].all()), r                     # every PICKED token was allowed
    lg = _teacher_logits(m, m.encoder(img), d, prefix, toks)
    want, st, bound = replay_greedy(rules, torch.from_numpy(lg), toks, state=start)
    before = states_before(rules, _np(toks), start)
    for t in range(n):
        _assert_picks(rules.mask(before[:, t], lg[:, t]), _np(toks)[:, t], t)
    assert np.array_equal(_np(state), st)
    assert bool(bound.any()), "no pick behind the prefixes met a disallowed arg-max: the test is vacuous"


def _closing_prefix_replay(m, d, rules, dist, img, prefix, n):
    """a closing prompted decode of n picks, replayed with rules.mask(remaining=, ended=, dist=) from rules.run of every prefix over the
    engine's teacher-forced logits: every pick by _assert_picks and allowed by the budgeted rule, the state returned is the replay's.
    -> (tokens (B, n'), per position: the states in front of it, the budgeted rows, the plain rows; final state, ended)"""
    lens = [len(p) for p in prefix]
    B = len(prefix)
    toks, state = _prompted(m, d, img, prefix, lens, n, rules=rules, close=True)
    assert m._engine.query(Q_LAST_PERSISTENT) == 0
    tk = _np(toks)
    lg = _teacher_logits(m, m.encoder(img), d, prefix, toks)
    st, ended = np.stack([rules.run(p[1:])[0] for p in prefix]), np.array([d.eos in p[1:] for p in prefix])
    trace = []
    for t in range(tk.shape[1]):
        row = rules.mask(st, lg[:, t], remaining=n - t, ended=ended, dist=dist)
        _assert_picks(row, tk[:, t], t)
        assert bool(rules.allowed(st, remaining=n - t, ended=ended, dist=dist)[np.arange(B), tk[:, t]].all()), t
        trace.append((st.copy(), row, rules.mask(st, lg[:, t])))
        st, _ = rules.step(st, tk[:, t])
        ended = ended | (tk[:, t] == d.eos)
    assert np.array_equal(_np(state), st)
    return tk, trace, st, ended


def test_forced_prefix_into_the_trap_and_past_the_budget():
    """closing, rules_close_start_kernel with prefix lengths: row 0's prefix ends in trap's state 2 (no way to eos: the plain rule from there,
    whatever is left), row 1's prefix opens to depth 12 with 3 picks left (D = 5 > R: distance-reducing picks only, the row ends open)"""
    d, sd, m, rules = _case("trap", 64, max_batch=2, max_len=32)
    dist = rules.close_dist(d.eos)
    dd = np.asarray(dist)
    img = rgb_images(2, 48, 64, 96).cuda()
    prefix = [[d.bos] + _path(rules, [(2, 0), (0, 2)]), [d.bos] + _path(rules, [(2, 0)] * 6)]
    start = np.stack([rules.run(p[1:])[0] for p in prefix])
    assert start.tolist() == [[2, 2], [0, 12]] and int(dd[2, 2]) == int(R.CLOSE_INF) and int(dd[0, 12]) == 5
    n = 3
    tk, trace, st, ended = _closing_prefix_replay(m, d, rules, dist, img, prefix, n)
    assert tk.shape == (2, n)
    for t, (s0, row, plain) in enumerate(trace):
        assert np.array_equal(row[0], plain[0])                                      # the trapped row: the plain rule's row
        nst, _ = rules.step(s0, tk[:, t])
        assert int(dd[nst[1, 0], nst[1, 1]]) == int(dd[s0[1, 0], s0[1, 1]]) - 1, t   # row 1: one step nearer at every pick
    assert not np.array_equal(trace[0][1][1], trace[0][2][1]), "the budget masked nothing on the open row"
    assert st[0, 0] == 2 and not ended[1] and d.eos not in tk[1].tolist()


def test_forced_prefix_wide_closing_from_the_upper_half():
    """closing under wide, V 1100 (all 2048 nodes staged behind a prefix): row 0's prefix -- +127, +127 -- stands at depth 254 in state 2
    with 2 picks left (D = 4 > R: distance-reducing picks only, ends open); row 1's -- +127, +1, a neutral token into state 4 -- at depth
    128 with exactly D = dist[4][128] picks left: it closes with its last pick, through the -128 that only state 4 has"""
    d, sd, m, rules = _case("wide", 1100, max_batch=2, max_len=32)
    dist = rules.close_dist(d.eos)
    dd = np.asarray(dist)
    img = rgb_images(2, 48, 64, 97).cuda()
    prefix = [[d.bos] + _path(rules, [(127, 1), (127, 2)]), [d.bos] + _path(rules, [(127, 1), (1, 2), (0, 4)])]
    start = np.stack([rules.run(p[1:])[0] for p in prefix])
    assert start.tolist() == [[2, 254], [4, 128]]
    n = int(dd[4, 128])
    assert 2 <= n < int(dd[2, 254]) and int(dd[4, 128]) != int(dd[0, 128]), (n, dd[2, 254], dd[0, 128])
    tk, trace, st, ended = _closing_prefix_replay(m, d, rules, dist, img, prefix, n)
    assert tk.shape == (2, n)
    for t, (s0, row, plain) in enumerate(trace):
        nst, _ = rules.step(s0, tk[:, t])
        for r in range(2):
            if tk[r, t] != d.eos:
                assert int(dd[nst[r, 0], nst[r, 1]]) == int(dd[s0[r, 0], s0[r, 1]]) - 1, (r, t)   # both rows: one step nearer at every pick
        assert not np.array_equal(row, plain), "the budget masked nothing"
    assert not ended[0] and d.eos not in tk[0].tolist() and st[0, 1] > 0
    assert ended[1] and tk[1, -1] == d.eos and close_ref.closed_rows(rules, [prefix[1][1:] + tk[1].tolist()], d.eos) == [True]
    assert zoo.events(rules, tk[1:], state0=start[1:])[0].max_need == 128, "the closing row did not take the -128"


# ---- e. beam search ------------------------------------------------------------------------------------------------------------------------
_REFS = {}


def _beam_case(name, vocab, images=2, **kw):
    key = (name, vocab, images, tuple(sorted(kw.items())))
    if key not in _REFS:
        d = _tiny(vocab)
        rules = MAKE[name](vocab, d.eos, (d.bos, d.pad), **kw)
        _REFS[key] = (_Ref(d, biased_sd(d, rules, 3, BIAS[name]), rgb_images(images, 48, 64, 42)), rules)
    return _REFS[key]


def _beam_model(ref, k, dtype="fp32"):
    _, _, m = build(ref.d, sd=ref.sd, dtype=dtype, max_batch=ref.img.shape[0] * k)
    m.rules_beam = True
    return m


@pytest.mark.parametrize("name,vocab,k", [("skew", 64, 3), ("skew", 1100, 3), ("wide", 64, 5)])
def test_beam_every_step_is_the_float64_replay(name, vocab, k):
    """beam_select_rules_kernel (V = 64: the register path, 1100: the general path) and beam_finish_rules_kernel: test_gpu_beam_rules's
    per-step float64 replay; every slot's rule_state is rules.run of that slot's own tokens"""
    N = 12
    ref, rules = _beam_case(name, vocab)
    m = _beam_model(ref, k)
    m.eos_token = None
    img = ref.img.cuda()
    states, beams = _states(m, img, k, range(1, N + 1), rules, return_logp=True)
    rep = br.replay_pairs(ref.s64, ref.enc64, ref.d.bos, None, states, range(N), _eps_fp32, logp_of=_masked_logp_of(ref, rules, None))
    assert rep.steps == N
    free = m.beam_search(img, k, N)
    assert not torch.equal(beams[N].tokens, free.tokens), "the rules never moved the search: nothing was tested"
    split = 0
    for n in range(1, N + 1):
        assert _check_live_beams(rules, beams[n], None, f"n={n}") == 2 * k or n == 1
        st = _np(beams[n].rule_state)
        live = np.isfinite(_np(beams[n].scores))
        split += sum(len({int(s) for s in st[b, live[b], 0]}) >= 2 for b in range(2))
    ev = zoo.events(rules, _np(beams[N].tokens).reshape(2 * k, N))
    print(f"\n[zoo] beam {name} V={vocab} k={k}: {split} (step, image) pairs with live beams in different states; deep close "
          f"{any(e.deep_close for e in ev)}, clamp at 0 {any(e.clamp_zero for e in ev)}, largest need {max(e.max_need for e in ev)}")
    assert split >= 1, "the live beams of an image always stood in one state: the state table was reordered together with nothing that differs"
    assert any(e.deep_close for e in ev), "no beam holds a delta <= -2 token"


@pytest.mark.parametrize("name,vocab", [("skew", 64), ("skew", 1100), ("trap", 64), ("trap", 1100)])
def test_closing_beam_search_is_the_float64_search(name, vocab):
    """beam_select_close_kernel, register and LDS paths: test_gpu_rules_close's comparison -- the final beams of beam_ref.search64 over the
    float64 log-probabilities under the budgeted mask, scores within beam_ref.eps_fp32 -- with distances that depend on the state; trap:
    the budget is on at every position, and no live beam stands in state 2"""
    N, k = 12, 3
    ref, rules = _beam_case(name, vocab)
    d = ref.d
    dist = rules.close_dist(d.eos)
    m = _beam_model(ref, k)
    img = ref.img.cuda()

    def logp_of(tokens):
        tokens = np.asarray(tokens, np.int64)
        B, kk, n = tokens.shape
        flat = tokens.reshape(B * kk, n).tolist()
        state = np.stack([rules.run(row)[0] for row in _cut(flat, d.eos)])
        ended = np.array([d.eos in row for row in flat])
        ok = rules.allowed(state, remaining=N - n, ended=ended, dist=dist)
        return np.where(ok.reshape(B, kk, -1), ref.logp(tokens), -np.inf)

    want = br.search64(logp_of, 2, k, d.eos, N)
    res = m.beam_search(img, k, N, rules=rules, close=True, return_logp=True)
    assert m._engine.query(Q_LAST_PERSISTENT) == 0
    tok, sc, ln, st = (_np(x) for x in (res.tokens, res.scores, res.lengths, res.rule_state))
    n = tok.shape[2]
    assert n <= N and n in want
    wt, ws = want[n]
    live = np.isfinite(sc)
    assert live.any(1).all() and np.array_equal(live, np.isfinite(ws))
    assert np.array_equal(tok[live], wt[live])
    assert float(np.abs(sc[live] - ws[live]).max()) < br.eps_fp32(sc[live])
    seen = set()
    for b in range(2):
        for r in range(k):
            if live[b, r]:
                row = tok[b, r, :ln[b, r]].tolist()
                assert row[-1] == d.eos and d.eos not in row[:-1], (b, r, row)
                fin, ok = rules.run(row)
                assert bool(ok.all()) and fin[1] == 0 and st[b, r].tolist() == fin.tolist(), (b, r)
                seen |= set(zoo.events(rules, row)[0].states)
                if name == "trap":
                    assert st[b, r, 0] != 2 and 2 not in zoo.events(rules, row)[0].states, (b, r)
    if name == "skew":                                             # (trap's two open states are left to the greedy cases: its beams close from state 0)
        assert len(seen) >= 2, "every live beam stood in state 0 throughout"
    off = m.beam_search(img, k, N, rules=rules, close=False, return_logp=True)
    assert not torch.equal(off.tokens[..., :n], res.tokens), "the budget never moved the search"
    if name == "trap":
        trapped = [2 in zoo.events(rules, r)[0].states for r in _cut(_np(off.tokens).reshape(2 * k, -1), d.eos)]
        print(f"\n[zoo] closing beam trap V={vocab}: {sum(trapped)} of {2 * k} beams of the plain constrained search enter state 2")
        assert any(trapped), "the plain constrained search never enters state 2: the trap was not in the way"


def test_closing_beam_search_bf16_paths_and_budget():
    """bf16, skew, V 64, k 3, as test_gpu_shapes.test_shape_matrix_beam_search_bf16_latent compares: each returned beam's score against the
    float64 score of its own token path -- a path the budgeted mask allows at every position (exact), ending at an allowed eos (exact).
    The bound is 1.5 x the same error of the same model and images with rules_beam off, measured here (the margin the suite uses for
    its bf16 calibration).  Measured on MI355X: 0.0329 under rules and budget, 0.0429 with rules_beam off (bound 0.0644)."""
    N, k = 12, 3
    ref, rules = _beam_case("skew", 64)
    d = ref.d
    dist = rules.close_dist(d.eos)
    m = _beam_model(ref, k, dtype="bf16")
    img = ref.img.cuda()

    def path_error(res):
        tok, sc, ln = (_np(x) for x in (res.tokens, res.scores, res.lengths))
        live = np.isfinite(sc)
        path = np.zeros(sc.shape)
        for t in range(tok.shape[2]):
            lp = ref.logp(tok[:, :, :t])                            # (B, k, V) float64 behind every beam's first t tokens
            path += np.where(t < ln, np.take_along_axis(lp, tok[:, :, t:t + 1], 2)[..., 0], 0.0)
        return float(np.abs(sc.astype(np.float64) - path)[live].max()), tok, ln, live

    res = m.beam_search(img, k, N, rules=rules, close=True)
    assert m._engine.query(Q_LAST_PERSISTENT) == 0
    err, tok, ln, live = path_error(res)
    st = _np(res.rule_state)
    assert live.any(1).all()
    seen = set()
    for b in range(2):
        for r in range(k):
            if not live[b, r]:
                continue
            row = tok[b, r, :ln[b, r]].tolist()
            assert ln[b, r] <= N and row[-1] == d.eos and d.eos not in row[:-1], (b, r, row)          # ends at an eos ...
            fin, ok = rules.run(row)
            assert bool(ok.all()) and fin[1] == 0 and st[b, r].tolist() == fin.tolist(), (b, r)       # ... that the rules allow
            for t, s0 in enumerate(states_before(rules, np.asarray([row]))[0]):                       # ... along a path the budget allows
                assert bool(rules.allowed(s0[None], remaining=N - t, ended=[False], dist=dist)[0, row[t]]), (b, r, t)
            seen |= set(zoo.events(rules, row)[0].states)
    assert len(seen) >= 2, "every live beam stood in state 0 throughout"
    m.rules_beam = False
    base, _, _, _ = path_error(m.beam_search(img, k, N))
    print(f"\n[zoo] bf16 closing beam skew V=64 k=3: max |score - float64 path score| {err:.5f} under rules and budget, {base:.5f} with "
          f"rules_beam off; bound {1.5 * base:.5f}")
    assert err < 1.5 * base, (err, base)


# ---- f. rows that move ---------------------------------------------------------------------------------------------------------------------
def _open_eos_skew(d):
    """skew with eos allowed at depth 0 in every state, so that rows do finish"""
    return zoo.skew(d.vocab, d.eos, (d.bos, d.pad), eos_states=(0, 1, 2))


@pytest.mark.parametrize("close", [False, True])
def test_row_stop_with_compactions_equals_every_image_alone(close):
    """gpu_harness.stop_case with a compaction every other position, under skew: a row's (state, depth) follows it through the moves -- every
    third row is the image decoded alone, tokens and state.  Guard: the engine looks at its finished rows every other position and moves the
    live ones four positions later, i.e. in front of a position 6, 10, 14, ...; at each of those with finished rows behind it and three or
    more rows still running, one of the running rows stands in a state other than 0."""
    d, sd, img = stop_case(bias=0.0)                                # (with the case's own eos bias every row ends at position 0 under skew)
    _, _, m = build(d, sd=sd, max_batch=40, env=STOP_ENV)
    img = img.cuda()
    rules = _open_eos_skew(d)
    with knobs(TXO_PERSIST=0):
        toks, state = m.generate(img, 40, stop="row", rules=rules, close=close)
    assert m._engine.query(Q_LAST_COMPACTIONS) >= 1 and m._engine.query(Q_LAST_PERSISTENT) == 0
    tk = _np(toks)
    n = tk.shape[1]
    if close:
        assert all(close_ref.closed_rows(rules, tk, d.eos))
    for r in range(0, 40, 3):
        t1, s1 = m.generate(img[r:r + 1], 40, stop="row", rules=rules, close=close)
        k = min(n, t1.shape[1])
        assert torch.equal(toks[r, :k], t1[0, :k]) and bool((toks[r, k:] == d.pad).all()), r
        assert torch.equal(state[r], s1[0]), r
        row = tk[r].tolist()
        st, ok = rules.run(row[:row.index(d.eos) + 1 if d.eos in row else n])       # a finished row froze its state behind its eos
        assert bool(ok.all()) and state[r].tolist() == st.tolist(), r
    first = np.array([row.index(d.eos) if d.eos in row else n for row in tk.tolist()])
    before = states_before(rules, np.where(tk == d.pad, d.eos, tk))                 # (only the states in front of a row's eos are read)
    moves = [p for p in range(6, n, 4) if (first < p - 4).any() and (first >= p).sum() >= 3]
    assert moves, "no position at which rows moved while three were running: the test is vacuous"
    for p in moves:
        running = first >= p
        assert bool((before[running, p, 0] != 0).any()), f"every row running at position {p} stands in state 0: nothing that differs moved"
    print(f"\n[zoo] row stop close={close}: {n} positions, {m._engine.query(Q_LAST_COMPACTIONS)} compactions, moves checked in front of {moves}")


def test_two_row_ranges_equal_every_image_alone():
    """fp32, 40 rows forced onto two ranges (TXO_LANES=2), the same rule set, plain and closing: rows 0, 19, 20 and 39 are the image alone"""
    d, sd, m = build(_tiny(64), seed=3, max_batch=40)
    rules = _open_eos_skew(d)
    img = rgb_images(40, 32, 48, 81).cuda()
    for close in (False, True):
        m.eos_token = d.eos if close else None
        with knobs(TXO_LANES=2):
            toks, logp, state = m.generate(img, 12, return_logp=True, rules=rules, close=close)
            assert m._engine.query(Q_LAST_ROW_RANGES) == 2
        if close:
            assert all(close_ref.closed_rows(rules, _np(toks), d.eos))
        seen = set()
        for r in (0, 19, 20, 39):
            t1, l1, s1 = m.generate(img[r:r + 1], 12, return_logp=True, rules=rules, close=close)
            k = min(toks.shape[1], t1.shape[1])
            assert k >= 1 and torch.equal(toks[r, :k], t1[0, :k]) and torch.equal(logp[r, :k], l1[0, :k]), (close, r)
            if not close:
                assert torch.equal(state[r], s1[0]), r
            seen |= set(zoo.events(rules, _cut(_np(toks[r:r + 1]), d.eos)[0])[0].states)
        assert len(seen) >= 2, "the four rows stood in state 0 throughout"


# ---- g. the brace rule of the 1k vocabulary, with logits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("close", [False, True])
def test_brace1k_tokens_are_the_replay(close):
    """test_gpu_rules.test_brace_rule_end_to_end's model and bias (plus one towards tokens that leave the text escaped, so that state 1 is
    visited), greedy, with the logits: a wrong but balanced pick does not pass"""
    tk = zoo.tok1k()
    d = _tiny(1000, max_len=32)
    rules = zoo.brace1k()
    sd = synth.synth_state_dict(d, 13)
    b = sd["decoder.net.to_logits.bias"].copy()
    b[[v for v in range(997) if R.token_braces(tk.vocab[v], False)[0] > 0]] += 1.5
    b[[d.eos, d.bos, d.pad]] += 1.0
    b[[v for v in range(997) if R.token_braces(tk.vocab[v], False)[2]]] += 1.5          # ... and towards tokens that end in an odd run of backslashes
    sd["decoder.net.to_logits.bias"] = b
    _, _, m = build(d, sd=sd, max_batch=4)
    if not close:
        m.eos_token = None
    img = rgb_images(4, 48, 64, 70).cuda()
    toks, logits, state = m.generate(img, 32, return_logits=True, rules=rules, close=close)
    t_np = _np(toks)
    if close:
        dist = rules.close_dist(d.eos)
        rows, st, ended = close_ref.replay(rules, dist, _np(logits.float()), t_np, 32)
        assert np.array_equal(t_np, rows.argmax(2)) and bool(ended.all())
        for row in _cut(t_np, d.eos):
            s = rules_ref.scan(tk.vocab, row, 64, d.eos)
            assert s.low == 0 and s.eos_depths == [0] and not any(s.disallowed), row
    else:
        want, st, bound = replay_greedy(rules, logits, toks)
        assert np.array_equal(t_np, want) and bool(bound.any())
        for r, row in enumerate(t_np.tolist()):
            s = rules_ref.scan(tk.vocab, row, 64, d.eos)
            assert state[r].tolist() == [int(s.odd), s.depth], r
    assert np.array_equal(_np(state), st)
    before = states_before(rules, t_np)
    odd = np.argwhere(before[..., 0] == 1)
    assert odd.size, "no row stood in state 1 (an odd run of backslashes) at a pick: the test is vacuous"
    assert any(not np.array_equal(*rules.allowed(np.array([[1, before[b, t, 1]], [0, before[b, t, 1]]], dtype=np.int32))) for b, t in odd)


# ---- the engine's table --------------------------------------------------------------------------------------------------------------------
def test_engine_tables_are_close_dist():
    """csrc/rules_close.h through the engine, as test_gpu_rules_close.test_engine_table_is_close_dist reads it: the full 2048-node table, the
    1280-node one, the one with a partial last piece, and the one with an unreachable state"""
    for vocab in (64, 1100):
        d, sd, m = build(_tiny(vocab), seed=3, max_batch=1)
        for make, kw in ((zoo.wide, {}), (zoo.wide, dict(S=5)), (zoo.wide, dict(S=3, depth_max=100)), (zoo.skew, {}), (zoo.trap, {})):
            rules = make(vocab, d.eos, (d.bos, d.pad), **kw)
            assert np.array_equal(m._engine.rules_close_dist(rules).numpy(), np.asarray(rules.close_dist(d.eos))), (vocab, make.__name__, kw)
