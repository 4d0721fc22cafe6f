"""No-GPU checks of the repeat guard's rule (texocr_amd/guard.py; include/texocr.h: txo_set_repeat_guard) against the brute-force
restatement tests/guard_ref.py, of the edge cases the definition names, of the fixture facts the GPU tests rest on, and of the host-side
argument refusals."""
import itertools
import os

import numpy as np
import pytest

import guard_ref
from texocr_amd import guard

HERE = os.path.dirname(os.path.abspath(__file__))


def test_exhaustive_short_histories_against_the_brute_force():
    """every history over a 3-letter alphabet up to length 10, P <= 4, R <= 3, with and without an eos among the letters"""
    n_banned = 0
    for n in range(0, 11):
        for h in itertools.product(range(3), repeat=n):
            for P in range(1, 5):
                for R in range(1, 4):
                    want = guard_ref.banned(h, P, R, None, vocab=3)
                    assert guard.banned(h, P, R) == want, (h, P, R)
                    n_banned += len(want)
            assert guard.banned(h, 4, 2, eos=2) == guard_ref.banned(h, 4, 2, 2, vocab=3), h
    assert n_banned > 10000                                      # (the comparison is not one of empty sets)


@pytest.mark.parametrize("p,R", [(1, 1), (1, 3), (2, 2), (3, 2), (4, 3), (16, 1), (16, 16), (3, 5)])
def test_off_by_one_pair(p, R):
    """m_p = R * p - 2 bans nothing, m_p = R * p - 1 bans h[n - p]: a history of one block repeated so that exactly that many trailing
    positions match (a different token in front stops the count)"""
    block = list(range(10, 10 + p))
    for m, banned in ((R * p - 2, False), (R * p - 1, True)):
        if m < 0:
            continue
        n = m + p                                                # m matching positions behind the first p tokens
        tail = [block[i % p] for i in range(n)]
        h = [99] + tail                                          # 99: the mismatch that ends the count
        got = guard.banned(h, p, R)
        assert got == guard_ref.banned(h, p, R), (m, h)
        assert (h[len(h) - p] in got) == banned, (m, h, got)


def test_eos_is_never_banned():
    h = [5, 5, 5]
    assert guard.banned(h, 1, 1) == {5} and guard.banned(h, 1, 1, eos=5) == set()
    assert guard.banned([7, 5, 7, 5, 7], 2, 2, eos=5) == set() and guard.banned([7, 5, 7, 5, 7], 2, 2, eos=7) == {5}
    assert guard_ref.banned([7, 5, 7, 5, 7], 2, 2, 5) == set()


def test_period_longer_than_the_history():
    assert guard.banned([], 16, 1) == set()
    assert guard.banned([3], 16, 1) == {3}                        # p = 1 only: p = 2 .. 16 exceed n
    assert guard.banned([3, 4], 16, 1) == {4}                     # p = 2 has no position i with i - 2 >= 0 to compare yet
    assert guard.banned([3, 4, 3], 16, 1) == {3, 4}               # p = 1 bans 3 (3 3), p = 2 bans 4 (4 3 | 4 3)
    for h in ([3, 4], [3, 4, 3]):
        assert guard.banned(h, 16, 1) == guard_ref.banned(h, 16, 1)
    assert guard.banned([3, 4], 16, 2) == set()


def test_two_periods_ban_the_same_token():
    h = [1] * 8                                                   # p = 1, 2 and 3 all ban token 1 under R = 2 (p = 4 would need 12 tokens)
    assert guard.banned(h, 4, 2) == {1} == guard_ref.banned(h, 4, 2)
    assert [p for p in range(1, 5) if guard_ref.ends_in_copies(h + [1], p, 3)] == [1, 2, 3]
    h = [2, 1, 1, 2, 1, 1, 2, 1]                                  # p = 3 bans 1 (2 1 1 three times); p = 1: the row ends in one 1 only
    assert guard.banned(h, 3, 2) == {1} == guard_ref.banned(h, 3, 2)
    h = [1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 1]                         # p = 2 and p = 4 both ban 2
    assert guard.banned(h, 4, 2) == {2}
    assert [p for p in range(1, 5) if guard_ref.ends_in_copies(h + [2], p, 3)] == [2, 4]


def test_hits_and_violations_per_row():
    rows = np.array([[4, 4, 4, 9, 9], [1, 2, 3, 4, 5]])
    assert guard.hits(rows, 1, 2) == [[2, 3], []]                 # behind "4 4" the set is {4} (positions 2 and 3: the run still stands at 3)
    assert guard.violations(rows, 1, 2) == [[2], []]
    assert guard.hits(rows[0], 1, 2) == [[2, 3]]
    for r in rows:
        assert guard_ref.hits(r, 1, 2) == guard.hits(r, 1, 2)[0] and guard_ref.violations(r, 1, 2) == guard.violations(r, 1, 2)[0]


def test_fixture_rows_loop():
    """the premise of the GPU tests: the reference's own greedy rows of tests/golden/tiny.npz violate (1, 1) five times each and (4, 2)
    once each; those of cfg1_b4_224x224.npz complete a third copy of a block of <= 4 tokens 3 - 4 times in 256 positions"""
    t = np.load(os.path.join(HERE, "golden", "tiny.npz"))["tokens"]
    assert t.shape == (2, 16)
    for impl in (lambda r, P, R: guard_ref.violations(r, P, R), lambda r, P, R: guard.violations(r, P, R)[0]):
        assert [len(impl(r, 1, 1)) for r in t] == [5, 5]
        assert [len(impl(r, 4, 2)) for r in t] == [1, 1]
    big = np.load(os.path.join(HERE, "golden", "cfg1_b4_224x224.npz"))["tokens"]
    assert big.shape == (4, 256)
    assert [len(v) for v in guard.violations(big, 4, 2)] == [3, 3, 4, 4]


def test_argument_refusals():
    assert guard.check(None) is None and guard.check((4, 3)) == (4, 3) and guard.check([16, 16], vocab=18) == (16, 16)
    for bad, text in [((0, 3), r"max_period is 0; it must be in \[1, 16\]"), ((17, 3), "max_period is 17"), ((-1, 1), "max_period is -1"),
                      ((4, 0), r"max_repeats is 0; it must be in \[1, 16\]"), ((4, 17), "max_repeats is 17"),
                      ((4,), "must be a pair of integers"), (5, "must be a pair of integers"), ((1.5, 2), "must be a pair of integers"),
                      ((True, 2), "must be a pair of integers")]:
        with pytest.raises(ValueError, match="repeat guard: .*" + text):
            guard.check(bad)
    with pytest.raises(ValueError, match=r"repeat guard: the vocabulary has 6 entries; it needs more than max_period \+ 1 = 6"):
        guard.check((5, 1), vocab=6)
    assert guard.check((4, 1), vocab=6) == (4, 1)
