"""No-GPU checks of tests/rule_zoo.py: every member validates, its distance table is the brute-force search's where that search is quick,
and the structural facts tests/test_gpu_rule_zoo.py relies on -- rows and distances that differ by state, deltas of -2 and below, a
token that clamps at 0, an unreachable state, the full 2048-node table and one whose last 16-byte piece is partial -- hold.  (The full
`wide` table against the one csrc/rules_close.h computes is in the GPU file: the engine is the only route to that header.)"""
import numpy as np
import pytest

import close_ref
import rule_zoo as zoo
from texocr_amd import rules as R

INF = int(R.CLOSE_INF)


def _special(V):
    return V - 3, (V - 2, V - 1)                                  # eos, (bos, pad): the ids of the tests' tiny Dims


MEMBERS = [("skew", zoo.skew, {}), ("trap", zoo.trap, {}), ("wide", zoo.wide, {}), ("wide5", zoo.wide, dict(S=5)),
           ("wide3", zoo.wide, dict(S=3, depth_max=100))]


@pytest.mark.parametrize("V", [64, 67, 1100])
@pytest.mark.parametrize("name,make,kw", MEMBERS)
def test_members_validate_and_differ_by_state(name, make, kw, V):
    eos, banned = _special(V)
    rules = make(V, eos, banned, **kw).validate(V)
    need, delta, nxt, flags = R.unpack(rules.table)
    assert bool((flags[:, list(banned)] == R.BAN).all())
    assert bool((flags[0, eos] == R.ONLY_AT_ZERO)) and bool((flags[1:, eos] != 0).any())
    for s in range(1, rules.n_states):
        assert not np.array_equal(rules.table[s], rules.table[0]), s                 # no state is a copy of state 0
    assert len({tuple(r) for r in rules.table.tolist()}) == rules.n_states
    deep = (delta <= -2) & (need < -delta) & (flags == 0)
    assert deep.any(), "no token with delta <= -2 that clamps at depth 0"
    assert bool(((delta <= -3) & (need == -delta) & (flags == 0)).any())             # ... and one whose need is >= 2
    dist = rules.close_dist(eos)
    d = np.asarray(dist)
    assert int(d[0, 0]) == 1
    assert any(not np.array_equal(d[s], d[0]) for s in range(1, rules.n_states)), "dist is the same in every state"
    if name == "skew":
        assert dist.dist_max >= 6 and not dist.any_inf
    if name == "trap":
        assert dist.any_inf and bool((d[2] == INF).all()) and bool((d[:2] != INF).all())
        assert bool((nxt[2] == 2).all()) and bool(((nxt[:2] == 2) & (flags[:2] == 0)).any())   # tokens into state 2 are ordinary tokens
    if name.startswith("wide"):
        assert not dist.any_inf
        assert d.size == {"wide": 2048, "wide5": 1280, "wide3": 303}[name]
        assert (d.size % 8 != 0) == (name == "wide3")
        assert int(delta.min()) == -(rules.depth_max // 2 + 1) and int(delta.max()) == rules.depth_max // 2
    if name == "wide":
        assert int(delta.min()) == -128 and int(delta.max()) == 127 and int(need.max()) == 128


@pytest.mark.parametrize("name,make,V,kw", [("skew", zoo.skew, 64, {}), ("trap", zoo.trap, 64, {}),
                                            ("wide", zoo.wide, 18, dict(S=3, depth_max=15)), ("wide", zoo.wide, 18, dict(S=8, depth_max=9))])
def test_close_dist_is_the_brute_force_search(name, make, V, kw):
    eos, banned = _special(V)
    rules = make(V, eos, banned, **kw)
    assert np.array_equal(np.asarray(rules.close_dist(eos)), close_ref.brute_dist(rules, eos))


def test_brace1k_has_two_rows_that_differ():
    rules = zoo.brace1k()
    assert rules.table.shape == (2, 1000) and not np.array_equal(rules.table[0], rules.table[1])
    assert np.array_equal(rules.table, R.brace_rules(zoo.tok1k(), depth_max=64).table)
    ok = rules.allowed(np.array([[0, 0], [1, 0]], dtype=np.int32))
    assert not np.array_equal(ok[0], ok[1])                       # the masks of the two states differ at one depth


def test_by_delta_reads_state_rows():
    rules = zoo.skew(64, 61, (62, 63))
    for s in range(3):
        for dl in (+2, -3, -2):
            ids = zoo.by_delta(rules, dl, state=s)
            assert all(R.unpack(rules.table[s, v])[1] == dl for v in ids)
            assert bool(ids) == (dl == 2 or s == 0 or (dl == -2 and s == 1))
    assert set(zoo.by_delta(rules, -2, lo=-3)) == set(zoo.by_delta(rules, -2)) | set(zoo.by_delta(rules, -3))


def test_events_on_hand_written_sequences():
    rules = zoo.skew(64, 61, (62, 63))
    # state 0: id % 7 = 0 open, 1 open two, 2 close, 3 close three, 4 drop, 5 / 6 neutral; next = (id + s) % 3, a lowering token stays
    assert [R.unpack(rules.table[0, v])[1].item() for v in range(7)] == [1, 2, -1, -3, -2, 0, 0]
    e, = zoo.events(rules, [21, 42, 3])                           # open (21 % 3 == 0: stays in 0), open (42: stays), close three at depth 2: clamps
    assert e == zoo.Events((0, 0, 0, 0), True, True, False, 3, 2)
    e, = zoo.events(rules, [1, 7])                                # +2 -> state 1 (1 % 3), there 7 has class (7 + 2) % 7 = 2: close, stays in 1
    assert e == zoo.Events((0, 1, 1), False, False, False, 1, 2)
    e, = zoo.events(rules, [5, 5])                                # neutral 5: state 0 -> 2; there (5 + 4) % 7 = 2: a close at depth 0, disallowed, clamps, stays
    assert e == zoo.Events((0, 2, 2), False, True, False, 1, 0)
    e, = zoo.events(rules, [4])                                   # the drop at depth 0: clamps, need 0
    assert e == zoo.Events((0, 0), True, True, False, 0, 0)
    e, = zoo.events(rules, [1], state0=[[0, 11]])                 # +2 at depth 11 of 12: clamps at depth_max (only a forced token can)
    assert e == zoo.Events((0, 1), False, False, True, 0, 12)
    two = zoo.events(rules, [[21, 3], [5, 5]])
    assert two[0].clamp_zero and two[0].max_need == 3 and two[1].states == (0, 2, 2)
    for row, ev in zip([[21, 42, 3], [1, 7], [5, 5]], zoo.events(rules, [[21, 42, 3], [1, 7, 5], [5, 5, 5]])):
        st, _ = rules.run(row)
        assert ev.states[len(row)] == st[0]                       # the states are rules.run's
