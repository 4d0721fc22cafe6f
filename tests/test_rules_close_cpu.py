"""No-GPU checks of the closing decode's rule (texocr_amd/rules.py: TokenRules.close_dist / allowed(remaining=); include/texocr.h:
txo_set_rules_close): the distance table against a brute-force breadth-first search (tests/close_ref.py) and, for the brace rule of the 1k
vocabulary, against the byte scan of the shortest closing string; the two consequences the specification relies on, as random walks; the
unchanged default; the host-side refusals, the two symbols and the operator."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import close_ref
import rules_ref
from texocr_amd import rules as R
from texocr_amd.tokenizer import RegExTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = int(R.CLOSE_INF)


@pytest.fixture(scope="module")
def lib():
    from texocr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def tok1k():
    v = json.load(open(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab_1k.json")))
    return RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"])


def random_rules(rng, S, V, depth_max, kind):
    """a valid random table (token 0 of every state is always allowed); eos is V - 1.  kind 'deep': tokens with delta -2; 'stuck': the last
    state has no closing token and no eos; 'banned': eos is banned in state 0"""
    need, delta = rng.integers(0, 3, (S, V)), rng.integers(-1, 2, (S, V))
    nxt, flags = rng.integers(0, S, (S, V)), np.where(rng.random((S, V)) < 0.15, R.BAN, 0)
    need[:, 0], delta[:, 0], flags[:, 0] = 0, 0, 0
    eos = V - 1
    need[:, eos], delta[:, eos], flags[:, eos] = 0, 0, R.ONLY_AT_ZERO
    if kind == "deep":
        delta[:, 1], need[:, 1], flags[:, 1] = -2, rng.integers(0, 3, S), 0
    if kind == "stuck":
        delta[S - 1] = np.abs(delta[S - 1])
        flags[S - 1, eos] = R.BAN
        nxt[S - 1] = S - 1
        need[S - 1, 0], delta[S - 1, 0], flags[S - 1, 0] = 0, 0, 0
    if kind == "banned":
        flags[0, eos] = R.BAN
    return R.TokenRules(R.pack(need, delta, nxt, flags), depth_max).validate(V), eos


CASES = [(S, V, dm, kind, seed) for seed, (S, V, dm) in enumerate([(1, 4, 1), (2, 7, 3), (3, 12, 4), (2, 12, 2), (3, 5, 4)])
         for kind in ("plain", "deep", "stuck", "banned")]


@pytest.mark.parametrize("S,V,depth_max,kind,seed", CASES)
def test_close_dist_is_the_brute_force_search(S, V, depth_max, kind, seed):
    rules, eos = random_rules(np.random.default_rng(100 + seed), S, V, depth_max, kind)
    got = rules.close_dist(eos)
    want = close_ref.brute_dist(rules, eos)
    assert got.dtype == np.int32 and got.shape == (S, depth_max + 1) and np.array_equal(np.asarray(got), want), (got, want)
    finite = want[want != INF]
    assert got.eos == eos and got.dist_max == (int(finite.max()) if finite.size else 0) and got.any_inf == bool((want == INF).any())
    if kind == "stuck" and S > 1:
        assert bool((want[S - 1] == INF).all())                   # no way out of the last state
    if kind == "banned" and S == 1:
        assert bool((want == INF).all())
    assert bool((np.asarray(rules.close_dist(-1)) == INF).all()) and bool((np.asarray(rules.close_dist(V)) == INF).all())


def test_brace_rule_distances_are_the_shortest_closing_strings(tok1k):
    """dist[0][d] of the 1k brace rule against tests/rules_ref.py's byte scan: a dynamic program over depths whose only oracle is the scan
    of d open braces followed by one token, and the scan of the closing string the table itself walks"""
    depth_max, eos = 12, tok1k.special_tokens["<EOS>"]
    rules = R.brace_rules(tok1k, depth_max=depth_max).validate()
    dist = rules.close_dist(eos)
    opener = next(v for v, b in tok1k.vocab.items() if b == b"{")
    best = {}
    for d in range(depth_max + 1):
        cand = []
        for v in tok1k.vocab:
            s = rules_ref.scan(tok1k.vocab, [opener] * d + [v], depth_max, eos, banned=(tok1k.special_tokens["<BOS>"], tok1k.special_tokens["<PAD>"]))
            if s.disallowed[-1] or s.odd:
                continue
            if v == eos:
                cand.append(1)
            elif s.depth < d:
                cand.append(1 + best[s.depth])
        best[d] = min(cand)
    assert [int(x) for x in dist[0]] == [best[d] for d in range(depth_max + 1)]
    assert best[0] == 1 and best[depth_max] <= depth_max + 1
    for d in range(depth_max + 1):                                # the string the table walks: every token allowed, eos at depth 0
        st, row = np.array([[0, d]], dtype=np.int32), []
        while not row or row[-1] != eos:
            D = int(dist[st[0, 0], st[0, 1]])
            ok = rules.allowed(st, remaining=D, dist=dist)[0]
            assert ok.any()
            row.append(int(np.nonzero(ok)[0][0]))
            st, _ = rules.step(st, [row[-1]])
        s = rules_ref.scan(tok1k.vocab, [opener] * d + row, depth_max, eos)
        assert len(row) == best[d] and not any(s.disallowed) and s.eos_depths == [0] and s.depth == 0 and s.low == 0, (d, row)


@pytest.mark.parametrize("S,V,depth_max,kind,seed", CASES)
def test_random_walks_close_inside_the_budget(S, V, depth_max, kind, seed):
    """uniform picks from allowed(remaining=R): started with dist <= R the walk commits an allowed eos within R picks; started with
    dist > R the distance falls by one per pick"""
    rng = np.random.default_rng(200 + seed)
    rules, eos = random_rules(rng, S, V, depth_max, kind)
    dist = rules.close_dist(eos)
    walks = 0
    for s0 in range(S):
        for d0 in range(depth_max + 1):
            D0 = int(dist[s0, d0])
            if D0 == INF:
                continue
            for R0 in (D0, D0 + 1, D0 + 5, max(D0 - 1, 1), 1):
                st, ended = np.array([[s0, d0]], dtype=np.int32), False
                for t in range(R0):
                    D = int(dist[st[0, 0], st[0, 1]])
                    ok = rules.allowed(st, remaining=R0 - t, ended=[ended], dist=dist)[0]
                    assert ok.any() and not (ok & ~rules.allowed(st)[0]).any()          # never empty, never wider than the plain rule
                    v = int(rng.choice(np.nonzero(ok)[0]))
                    st, allowed = rules.step(st, [v])
                    assert bool(allowed[0])
                    if v == eos:
                        ended = True
                        break
                    if D0 > R0:
                        assert int(dist[st[0, 0], st[0, 1]]) == D - 1, (s0, d0, R0, t)
                assert ended == (D0 <= R0), (s0, d0, R0)
                walks += 1
    assert walks > 0 or kind in ("stuck", "banned")


def test_ended_and_infinite_rows_keep_the_plain_rule_and_the_default_is_unchanged():
    rules, eos = random_rules(np.random.default_rng(7), 3, 12, 4, "stuck")
    dist = rules.close_dist(eos)
    state = np.array([[s, d] for s in range(3) for d in range(5)], dtype=np.int32)
    plain = rules.allowed(state)
    inf_rows = np.asarray(dist)[state[:, 0], state[:, 1]] == INF
    assert inf_rows.any() and not inf_rows.all()
    got = rules.allowed(state, remaining=1, dist=dist)
    assert np.array_equal(got[inf_rows], plain[inf_rows]) and not np.array_equal(got[~inf_rows], plain[~inf_rows])
    assert np.array_equal(rules.allowed(state, remaining=1, ended=np.ones(len(state), dtype=bool), dist=dist), plain)
    # a table without an infinite entry, and more picks left than its largest distance: the plain rule
    free, eos2 = random_rules(np.random.default_rng(8), 2, 12, 3, "plain")
    d2 = free.close_dist(eos2)
    st2 = np.array([[s, d] for s in range(2) for d in range(4)], dtype=np.int32)
    if not d2.any_inf:
        assert np.array_equal(free.allowed(st2, remaining=d2.dist_max + 1, dist=d2), free.allowed(st2))
    # the arguments left out: exactly the old functions
    lg = np.random.default_rng(1).standard_normal((len(state), 12)).astype(np.float32)
    assert np.array_equal(rules.allowed(state, None, None, None), plain)
    assert np.array_equal(rules.mask(state, lg), np.where(plain, lg, R.MASKED))
    assert np.array_equal(rules.mask(state, lg, remaining=1, dist=dist), np.where(got, lg, R.MASKED))
    for kw in (dict(ended=[False]), dict(dist=dist)):
        with pytest.raises(ValueError, match="belong to remaining="):
            rules.allowed(state, **kw)
    with pytest.raises(ValueError, match="remaining= needs dist="):
        rules.allowed(state, remaining=3)
    with pytest.raises(ValueError, match="remaining= needs dist="):
        rules.allowed(state, remaining=3, dist=np.asarray(dist))


def test_host_side_refusals_of_close():
    """close= without rules= is refused by the one scope every entry goes through, before an engine is touched"""
    from texocr_amd.model import HipEngine

    class Stub:
        modes = HipEngine.modes
    with pytest.raises(ValueError, match="close=True needs rules="):
        with Stub().modes(close=True):
            pass
    with pytest.raises(ValueError, match="close must be False or True"):
        with Stub().modes(close=2):
            pass


def test_c_abi_refusals_without_gpu(lib):
    from texocr_amd import _lib
    assert lib.txo_set_rules_close(None, 1) == _lib.TXO_E_INVALID and "null engine" in lib.txo_last_error().decode()
    buf = (C.c_int32 * 4)()
    assert lib.txo_rules_close_dist(None, buf, 1, 4) == _lib.TXO_E_INVALID and "null" in lib.txo_last_error().decode()


def test_symbols_declared_bound_and_counted(lib):
    from texocr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "texocr.h")).read()
    for name, n_args in (("txo_set_rules_close", 2), ("txo_rules_close_dist", 4)):
        decl = re.search(r"^int " + name + r"\((.*?)\);", hdr, re.M | re.S).group(1)
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert len(decl.split(",")) == n_args == len(_lib.SYMBOLS[name][1])
    assert "#define TXO_CLOSE_INF 0x7fffffff" in hdr and INF == 0x7fffffff
    assert f"({len(_lib.SYMBOLS)} entry points)" in open(os.path.join(ROOT, "README.md")).read()


def test_op_registered_with_fake_impl():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from texocr_amd import ops
    from texocr_amd.config import Dims

    class Stub:
        dims, device = Dims(canvas=672), 0
    stub = Stub()
    eid = ops.register_engine(stub)
    try:
        assert hasattr(torch.ops.texocr, "set_rules_close")
        with FakeTensorMode():
            assert torch.ops.texocr.set_rules_close(eid, True) is None
            assert torch.ops.texocr.set_rules_close(eid, False) is None
    finally:
        ops.unregister_engine(eid)


def test_documents_state_the_guarantee_and_its_two_exceptions():
    for name in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "txo_set_rules_close" in text, name
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert re.search(r"infeasible prefix", readme) and re.search(r"dead beams", readme)
