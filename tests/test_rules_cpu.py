"""No-GPU checks of the constrained decode's rule (texocr_amd/rules.py; include/texocr.h: txo_set_token_rules): the brace automaton of the
1k vocabulary against a byte-by-byte scan of the decoded string (tests/rules_ref.py), the entry's packing, TokenRules.step against a
per-element loop, validate()'s refusals and the same refusals through the C ABI (the table is checked before an engine is looked at), the
two symbols and their operators."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import rules_ref
from texocr_amd import rules as R
from texocr_amd.tokenizer import RegExTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from texocr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def tok1k():
    v = json.load(open(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab_1k.json")))
    return RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"])


def test_pack_unpack_round_trip():
    rng = np.random.default_rng(0)
    need, delta = rng.integers(0, 256, 5000), rng.integers(-128, 128, 5000)
    nxt, flags = rng.integers(0, 256, 5000), rng.integers(0, 4, 5000)
    e = R.pack(need, delta, nxt, flags)
    assert e.dtype == np.int32
    for got, want in zip(R.unpack(e), (need, delta, nxt, flags)):
        assert np.array_equal(got, want)
    # the documented bit layout, by hand: need 3, delta -2, next 5, ONLY_AT_ZERO
    assert int(R.pack(3, -2, 5, R.ONLY_AT_ZERO)) == 3 | (0xfe << 8) | (5 << 16) | (1 << 25)
    assert int(R.pack(flags=R.BAN)) == 1 << 24
    for bad in (dict(need=256), dict(need=-1), dict(delta=128), dict(delta=-129), dict(next=256), dict(flags=4)):
        with pytest.raises(ValueError, match="token rules"):
            R.pack(**bad)


def _step_loop(rules, state, tokens):
    """the rule, element by element, from the module's documentation"""
    out, oks = [], []
    for (s, depth), t in zip(state.tolist(), tokens.tolist()):
        e = int(rules.table[s, t]) & 0xffffffff
        need, delta, nxt, flags = e & 0xff, (e >> 8) & 0xff, (e >> 16) & 0xff, e >> 24
        delta = delta - 256 if delta >= 128 else delta
        ok = not (flags & 1) and depth >= need and depth + delta <= rules.depth_max and (not (flags & 2) or depth == 0)
        out.append([nxt, min(max(depth + delta, 0), rules.depth_max)])
        oks.append(ok)
    return np.array(out, dtype=np.int32), np.array(oks)


def test_step_against_a_python_loop():
    rng = np.random.default_rng(1)
    S, V, dmax = 5, 37, 6
    table = R.pack(rng.integers(0, 4, (S, V)), rng.integers(-3, 4, (S, V)), rng.integers(0, S, (S, V)), rng.integers(0, 4, (S, V)))
    rules = R.TokenRules(table, dmax)
    state = np.stack([rng.integers(0, S, 4000), rng.integers(0, dmax + 1, 4000)], 1).astype(np.int32)
    tokens = rng.integers(0, V, 4000)
    got, ok = rules.step(state, tokens)
    want, wok = _step_loop(rules, state, tokens)
    assert np.array_equal(got, want) and np.array_equal(ok, wok)
    assert 0.05 < ok.mean() < 0.95                                # both verdicts occur
    allowed = rules.allowed(state)
    assert np.array_equal(allowed[np.arange(4000), tokens], ok)
    lg = rng.standard_normal((4000, V)).astype(np.float32)
    m = rules.mask(state, lg)
    assert m.dtype == np.float32 and np.array_equal(m[allowed], lg[allowed]) and bool((m[~allowed] == np.float32(-3.4e38)).all())


def test_ban_rule():
    r = R.ban(10, [2, 7]).validate(10)
    assert r.n_states == 1 and r.depth_max == 1
    st, ok = r.run([0, 2, 3, 7, 9])
    assert st.tolist() == [0, 0] and ok.tolist() == [True, False, True, False, True]


def test_brace_rules_equal_the_byte_scan(tok1k):
    """2000 random sequences of 1-40 tokens, half of them drawn only from tokens that contain a backslash or a brace: the automaton's final
    (s, depth) and its verdict on every token are the byte scan's"""
    dmax = 5                                                      # small enough for the cap to bind in the brace-heavy half
    rules = R.brace_rules(tok1k, depth_max=dmax).validate(1000)
    sp = tok1k.special_tokens
    eos, banned = sp["<EOS>"], (sp["<BOS>"], sp["<PAD>"])
    special = [v for v in range(1000) if any(c in tok1k.vocab[v] for c in b"\\{}")] + [eos]
    assert len(special) > 20
    rng = np.random.default_rng(2)
    verdicts = caps = odd_ends = 0
    for i in range(2000):
        n = int(rng.integers(1, 41))
        seq = rng.choice(special, n) if i % 2 else rng.integers(0, 1000, n)
        want = rules_ref.scan(tok1k.vocab, seq, dmax, eos, banned)
        st, ok = rules.run(seq)
        assert st.tolist() == [int(want.odd), want.depth], (i, seq.tolist())
        assert (~ok).tolist() == want.disallowed, (i, seq.tolist())
        assert bool((~ok).any()) == any(want.disallowed)
        verdicts += int((~ok).sum()); caps += int(want.depth == dmax); odd_ends += int(want.odd)
    print(f"\n[rules] {verdicts} refusals, {caps} sequences end at the cap, {odd_ends} end escaped")
    assert verdicts > 100 and caps > 20 and odd_ends > 5         # not vacuous: refusals, the cap and both states are reached


def test_brace_rules_by_hand():
    class Tk:
        vocab_size = 8
        special_tokens = {"<PAD>": 7, "<BOS>": 6, "<EOS>": 5}
        vocab = {0: b"a", 1: b"{", 2: b"}", 3: b"\\", 4: b"}{", 5: b"<EOS>", 6: b"<BOS>", 7: b"<PAD>"}
    r = R.brace_rules(Tk(), depth_max=2).validate(8)
    need, delta, nxt, flags = R.unpack(r.table)
    assert (need[0, 4], delta[0, 4]) == (1, 0)                    # "}{" dips one below its entry depth, net 0
    assert (need[1, 1], delta[1, 1], nxt[1, 1]) == (0, 0, 0)      # an escaped brace is text
    assert nxt[0, 3] == 1 and nxt[1, 3] == 0                      # a backslash flips the parity
    assert flags[0, 5] == R.ONLY_AT_ZERO and flags[0, 6] == R.BAN and flags[0, 7] == R.BAN
    st, ok = r.run([1, 1, 1, 2, 3, 2, 2, 5, 2, 5])                # {{ { (cap) } \ } (escaped) } <EOS> (depth 0) } (need) <EOS>
    assert ok.tolist() == [True, True, False, True, True, True, True, True, False, True]
    assert st.tolist() == [0, 0]


def test_validate_refusals():
    ok = R.pack(np.zeros((2, 6), dtype=np.int64))
    R.TokenRules(ok, 1).validate(6)
    with pytest.raises(ValueError, match=r"S is 9; the number of states must be in \[1, 8\]"):
        R.TokenRules(np.zeros((9, 6), dtype=np.int32), 4).validate()
    with pytest.raises(ValueError, match="S is 0"):
        R.TokenRules(np.zeros((0, 6), dtype=np.int32), 4).validate()
    for dm in (0, 256):
        with pytest.raises(ValueError, match=rf"depth_max is {dm}; it must be in \[1, 255\]"):
            R.TokenRules(ok, dm).validate()
    t = ok.copy(); t[1, 3] = R.pack(next=2)
    with pytest.raises(ValueError, match=r"rules\[1\]\[3\] has next = 2, not a state below S = 2"):
        R.TokenRules(t, 4).validate()
    t = ok.copy(); t[1] = R.pack(flags=[R.BAN, R.ONLY_AT_ZERO, 0, 0, R.BAN, 3], need=[0, 0, 1, 0, 0, 0], delta=[0, 0, 0, 1, 0, 0])
    with pytest.raises(ValueError, match="state 1 has no always-allowed token"):
        R.TokenRules(t, 4).validate()
    with pytest.raises(ValueError, match="V is 6 but the engine's vocabulary has 7 entries"):
        R.TokenRules(ok, 4).validate(7)


def test_c_abi_refusals_without_gpu(lib):
    """the same texts from txo_set_token_rules: the table is checked before the engine is looked at, so a null engine reaches every one of
    them but the vocabulary's (which needs an engine)"""
    from texocr_amd import _lib

    def call(table, depth_max, S=None):
        t = np.ascontiguousarray(table, dtype=np.int32)
        rc = lib.txo_set_token_rules(None, t.ctypes.data_as(C.c_void_p), t.shape[0] if S is None else S, t.shape[1], depth_max)
        return rc, lib.txo_last_error().decode()

    ok = R.pack(np.zeros((2, 6), dtype=np.int64))
    cases = [(np.zeros((9, 6)), 4, None), (ok, 4, 0), (ok, 0, None), (ok, 256, None)]
    t1 = ok.copy(); t1[1, 3] = R.pack(next=2)
    t2 = ok.copy(); t2[1] = R.pack(flags=[R.BAN, R.ONLY_AT_ZERO, 0, 0, R.BAN, 3], need=[0, 0, 1, 0, 0, 0], delta=[0, 0, 0, 1, 0, 0])
    cases += [(t1, 4, None), (t2, 4, None)]
    for table, dm, S in cases:
        rc, msg = call(table, dm, S)
        assert rc == _lib.TXO_E_INVALID and msg.startswith("token rules: "), msg
        shaped = np.zeros((S, 6), dtype=np.int32) if S is not None else table
        with pytest.raises(ValueError) as ei:
            R.TokenRules(shaped, dm).validate()
        assert str(ei.value) == msg                              # one text in both layers
    rc, msg = call(ok, 4)                                         # a good table, no engine
    assert rc == _lib.TXO_E_INVALID and "null engine" in msg
    assert lib.txo_set_token_rules(None, None, 0, 0, 0) == _lib.TXO_E_INVALID and "null engine" in lib.txo_last_error().decode()
    assert lib.txo_last_rule_state(None, None, 1, None) == _lib.TXO_E_INVALID and "null" in lib.txo_last_error().decode()


def test_symbols_declared_bound_and_counted(lib):
    from texocr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "texocr.h")).read()
    for name, n_args in (("txo_set_token_rules", 5), ("txo_last_rule_state", 4)):
        decl = re.search(r"^int " + name + r"\((.*?)\);", hdr, re.M | re.S).group(1)
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert len(decl.split(",")) == n_args == len(_lib.SYMBOLS[name][1])
    assert f"#define TXO_RULE_BAN (1 << 24)" in hdr and "#define TXO_RULE_ONLY_AT_ZERO (1 << 25)" in hdr
    assert f"({len(_lib.SYMBOLS)} entry points)" in open(os.path.join(ROOT, "README.md")).read()


def test_ops_registered_with_fake_impls():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from texocr_amd import ops
    from texocr_amd.config import Dims

    class Stub:
        dims, device = Dims(canvas=672), 0
    stub = Stub()
    eid = ops.register_engine(stub)
    try:
        assert hasattr(torch.ops.texocr, "set_token_rules") and hasattr(torch.ops.texocr, "last_rule_state")
        with FakeTensorMode():
            assert torch.ops.texocr.set_token_rules(torch.zeros((2, 1000), dtype=torch.int32), eid, 64) is None
            assert torch.ops.texocr.set_token_rules(None, eid, 0) is None
            st = torch.ops.texocr.last_rule_state(torch.empty((4, 9), dtype=torch.int64), eid)
            assert st.shape == (4, 2) and st.dtype == torch.int32
        with pytest.raises(ValueError, match="GPU tensor"):
            ops.last_rule_state(torch.zeros((2, 3), dtype=torch.int64), eid)
    finally:
        ops.unregister_engine(eid)


def test_documents_name_the_feature_and_its_two_limits():
    for name in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "txo_set_token_rules" in text, name
        assert re.search(r"beam", text) and re.search(r"may (still )?end open", text), name
