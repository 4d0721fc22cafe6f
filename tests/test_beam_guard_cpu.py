"""No-GPU checks of beam search under the repeat guard (tests/test_gpu_beam_guard.py has the GPU tests): tests/beam_guard_ref.py -- the
search in numpy over a table-driven toy model -- against brute-force enumeration of every sequence, free, under rules, and under rules with
a state whose only allowed token gets banned (the yield rule); guard.check's refusals through the beam calls; and what the new switch's
Python and C side answer without a device."""
import functools
import inspect
import itertools
import os
import re
import types

import numpy as np
import pytest
import torch

import beam_guard_ref as bgr
import beam_rules_ref as brr
import guard_ref
from texocr_amd import guard
from texocr_amd import rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, K, EOS = 5, 3, 4


def _free_rules():
    return None


def _ban_rules():
    """two states (next = id & 1): state 0 bans token 2, state 1 bans token 3"""
    ids = np.arange(V)
    rows = []
    for banned in (2, 3):
        flags = np.zeros(V, np.int64)
        flags[banned] = R.BAN
        rows.append(R.pack(next=ids & 1, flags=flags))
    return R.TokenRules(np.stack(rows), 1).validate(V)


def _one_token_rules():
    """state 0 allows everything but eos and sends token 1 to state 1; state 1 allows ONLY token 1 and stays: behind the first 1 the guard
    (1, 1) bans the one allowed token at every pick, and must yield"""
    ids = np.arange(V)
    f0 = np.zeros(V, np.int64)
    f0[EOS] = R.BAN
    f1 = np.where(ids == 1, 0, R.BAN)
    return R.TokenRules(np.stack([R.pack(next=(ids == 1).astype(np.int64), flags=f0), R.pack(next=np.ones(V, np.int64), flags=f1)]), 1).validate(V)


def _brute(table, rules, guard_pr, eos, n):
    """every sequence of length n -> (score, yields) by the definition, each on its own: the sum of the raw log-probabilities of its tokens up
    to and including its first eos; -inf if, at some position, the token is not in that position's pick set -- allowed (rules.run on the
    prefix) minus guard_ref.banned(prefix), or allowed alone where the difference is empty -- or a token behind the first eos is not eos"""
    out = {}
    for seq in itertools.product(range(V), repeat=n):
        cut = seq.index(eos) + 1 if eos in seq else n
        ok, total, last, yields = all(t == eos for t in seq[cut:]), 0.0, V, 0
        for i, t in enumerate(seq[:cut]):
            if rules is None:
                allowed = np.ones(V, bool)
            else:
                state, fine = rules.run(list(seq[:i]))
                ok = ok and bool(fine.all())
                allowed = rules.allowed(state[None])[0]
            pick = allowed & ~np.isin(np.arange(V), sorted(guard_ref.banned(list(seq[:i]), guard_pr[0], guard_pr[1], eos)))
            if not pick.any():
                pick, yields = allowed, yields + 1
            ok = ok and bool(pick[t])
            total += float(brr.log_softmax(table[last])[t])
            last = t
        out[seq] = (total if ok else -np.inf, yields)
    return out


@pytest.mark.parametrize("name,make,guard_pr,seed,bias", [("free", _free_rules, (1, 1), 0, {1: 2.0}), ("free", _free_rules, (2, 1), 1, {0: 1.5, 2: 1.5}),
                                                          ("ruled", _ban_rules, (2, 1), 2, {0: 1.5, 1: 1.5}), ("ruled", _ban_rules, (1, 2), 3, {1: 3.0}),
                                                          ("yield", _one_token_rules, (1, 1), 4, {1: 1.0})])
def test_search_is_the_brute_force_step_by_step(name, make, guard_pr, seed, bias):
    """every sequence of length <= 5 over 5 tokens scored on its own: a live beam's score is its sequence's, the beams at n + 1 are the k
    best of ALL sequences that extend a live beam at n, and no live beam holds a token outside its pick set.  The favoured tokens make the
    unguarded search repeat (asserted: the guard moves the beams)"""
    rng = np.random.RandomState(seed)
    table = rng.randn(V + 1, V)
    for t, off in bias.items():
        table[:, t] += off
    rules = make()
    N = 5
    states = bgr.search(table, rules, guard_pr, K, EOS, N)
    unguarded = bgr.search(table, rules, None, K, EOS, N)
    if rules is not None:                                          # the unguarded form is beam_rules_ref's search
        want = brr.search(table, rules, K, EOS, N)
        assert all(np.array_equal(want[n].tokens, unguarded[n].tokens) and np.array_equal(want[n].scores, unguarded[n].scores) for n in want)
    moved, yields = False, 0
    for n in range(max(states)):
        a, b = states[n], states[n + 1]
        brute = _brute(table, rules, guard_pr, EOS, n + 1)
        live_a = {tuple(t) for t, s in zip(a.tokens.tolist(), a.scores) if np.isfinite(s)}
        pool = sorted((s for q, (s, _) in brute.items() if q[:n] in live_a and np.isfinite(s)), reverse=True)
        live_b = np.isfinite(b.scores)
        assert int(live_b.sum()) == min(K, len(pool)), n
        np.testing.assert_allclose(b.scores[live_b], pool[:int(live_b.sum())], rtol=0, atol=1e-12)
        assert bool((b.scores[:-1] >= b.scores[1:]).all())
        for r in np.nonzero(live_b)[0]:
            seq = tuple(b.tokens[r].tolist())
            assert abs(brute[seq][0] - b.scores[r]) < 1e-12, (n, r)
            yields += brute[seq][1]
            cut = list(seq[:seq.index(EOS) + 1]) if EOS in seq else list(seq)
            if not brute[seq][1]:
                assert guard_ref.violations(cut, guard_pr[0], guard_pr[1], EOS) == [], (n, r, seq)
            if rules is not None:
                st, ok = rules.run(cut)
                assert bool(ok.all()) and b.rule_state[r].tolist() == st.tolist(), (n, r)
        moved = moved or (n + 1 in unguarded and not np.array_equal(unguarded[n + 1].tokens, b.tokens))
    assert moved, "the guard never changed a beam: nothing was tested"
    assert (yields > 0) == (name == "yield"), (name, yields)


def test_a_guard_that_cannot_bind_is_the_unguarded_search():
    """(16, 16) needs 16 committed tokens before its first ban: at 6 positions it is beam_ref.search64, free, and beam_rules_ref under rules"""
    import beam_ref as br
    table = np.random.RandomState(5).randn(V + 1, V)
    got = bgr.search(table, None, (16, 16), K, EOS, 6)
    want = br.search64(lambda tok: brr.toy_logp(table, tok[0])[None], 1, K, EOS, 6)
    assert max(got) == max(want)
    for n in want:
        assert np.array_equal(got[n].tokens, want[n][0][0]) and np.array_equal(got[n].scores, want[n][1][0]), n
    ruled, same = bgr.search(table, _ban_rules(), (16, 16), K, EOS, 6), brr.search(table, _ban_rules(), K, EOS, 6)
    assert all(np.array_equal(ruled[n].tokens, same[n].tokens) and np.array_equal(ruled[n].rule_state, same[n].rule_state) for n in same)
    # the arithmetic of the GPU test's premise: under (16, 16) a row of 15 committed tokens has no ban set, one of 16 may
    assert guard.hits(np.ones((1, 16), np.int64), 16, 16) == [[]] and guard.banned([1] * 16, 16, 16) == {1} == guard_ref.banned([1] * 16, 16, 16)


def test_keep_is_guard_refs_mask():
    rng = np.random.RandomState(1)
    for _ in range(50):
        h = rng.randint(0, 3, rng.randint(0, 9)).tolist()
        allowed = rng.rand(V) < 0.5
        allowed[rng.randint(V)] = True
        P, Rr = int(rng.randint(1, 4)), int(rng.randint(1, 3))
        keep, ban, yielded = bgr.keep(h, allowed, P, Rr, EOS)
        row, ban2, yielded2 = guard_ref.mask(np.zeros(V, np.float32), h, P, Rr, EOS, allowed)
        assert ban == ban2 == guard.banned(h, P, Rr, EOS) and yielded == yielded2 and np.array_equal(keep, row == 0)
        assert keep.any()


# ---- guard.check's refusals through the beam calls -------------------------------------------------------------------------------------
def test_guard_refusals_reach_the_beam_calls_in_the_same_words(monkeypatch):
    """OCRModel.beam_search and generate(beam=k) hand repeat_guard= to HipEngine.modes, which runs guard.check with the vocabulary before
    anything reaches the engine: the ValueError is guard.check's own, word for word.  (The scope's exit puts the guard of before back
    through the op: recorded here, there is no engine behind it.)"""
    from texocr_amd import model
    from texocr_amd.config import Dims
    calls, restored = [], []
    assert torch.ops.texocr.set_repeat_guard is not None
    monkeypatch.setattr(torch.ops.texocr, "set_repeat_guard", lambda eid, p, r: restored.append((p, r)))
    eng = types.SimpleNamespace(dims=Dims(canvas=672), id=0, max_batch=64, repeat_guard=None, token_rules=None, _ensure=lambda: None,
                                beam_search=lambda *a, **k: calls.append("beam_search"), generate_beam=lambda *a, **k: calls.append("generate_beam"))
    eng.set_repeat_guard = functools.partial(model.HipEngine.set_repeat_guard, eng)
    eng.modes = functools.partial(model.HipEngine.modes, eng)
    m = types.SimpleNamespace(_engine=eng, decoder=types.SimpleNamespace(max_len=32), eos_token=2)
    img = torch.zeros((1, 3, 16, 16))
    vocab = eng.dims.vocab
    for bad in ((0, 3), (17, 3), (4, 0), (4, 17), (4,), 5, (1.5, 2), (True, 2)):
        with pytest.raises(ValueError) as want:
            guard.check(bad, vocab)
        for call in (lambda: model.OCRModel.beam_search(m, img, 2, 8, repeat_guard=bad),
                     lambda: model.OCRModel.generate(m, img, 8, beam=2, repeat_guard=bad)):
            with pytest.raises(ValueError) as got:
                call()
            assert str(got.value) == str(want.value) and str(got.value).startswith("repeat guard: ")
    assert calls == [] and restored == [(0, 0)] * 16


# ---- the switch, where it needs no device ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from texocr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_c_abi_without_gpu(lib):
    from texocr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "texocr.h")).read()
    decl = re.search(r"^int txo_set_guard_beam\((.*?)\);", hdr, re.M | re.S).group(1)
    assert "txo_set_guard_beam" in _lib.SYMBOLS and hasattr(lib, "txo_set_guard_beam")
    assert len(decl.split(",")) == 2 == len(_lib.SYMBOLS["txo_set_guard_beam"][1])
    assert lib.txo_set_guard_beam(None, 1) == _lib.TXO_E_INVALID and "null" in lib.txo_last_error().decode()


def test_python_side_of_the_switch():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from texocr_amd import model, ops, wrapper
    from texocr_amd.config import Dims
    for fn in (model.create_model, wrapper.TeXOCRWrapper.__init__):
        assert inspect.signature(fn).parameters["guard_beam"].default is False
    assert isinstance(model.OCRModel.guard_beam, property) and isinstance(model.HipEngine.guard_beam, property)

    class Stub:
        dims, device = Dims(canvas=672), 0
    stub = Stub()                                                 # (the registry keeps a weak reference)
    eid = ops.register_engine(stub)
    try:
        with FakeTensorMode():
            assert torch.ops.texocr.set_guard_beam(eid, True) is None
    finally:
        ops.unregister_engine(eid)
    with pytest.raises(ValueError, match="guard_beam must be False or True"):
        model.HipEngine.guard_beam.fset(stub, 2)
    # the wrapper keeps its words without the switch
    w = types.SimpleNamespace(repeat_guard=(1, 1), model=types.SimpleNamespace(guard_beam=False))
    with pytest.raises(ValueError, match="repeat_guard is not available with decode='beam'"):
        wrapper.TeXOCRWrapper._guard(w, None, "beam")
    w.model.guard_beam = True
    assert wrapper.TeXOCRWrapper._guard(w, None, "beam") == {"repeat_guard": (1, 1)} and wrapper.TeXOCRWrapper._guard(w, False, "beam") == {}


def test_lds_refusal_arithmetic():
    """the dynamic LDS of the guarded selection, beams * (window * 4 + ceil(V / 32) * 4) bytes, against the 56 KB the entry allows: the test
    vocabularies are far inside it; at 8 beams under guard (16, 16) it is passed between 48 000 and 49 000 entries"""
    def need(k, vocab, P, Rr):
        return k * (((Rr + 1) * P - 1) * 4 + ((vocab + 31) // 32) * 4)
    assert need(8, 1100, 16, 16) == 9792 and need(5, 1000, 4, 3) == 940
    assert need(8, 48000, 16, 16) <= 56 * 1024 < need(8, 49000, 16, 16)
    hip = open(os.path.join(ROOT, "texocr_amd", "csrc", "beam_guard.h")).read()
    assert "BEAM_GUARD_LDS_MAX = 65536 - 8192" in hip and "return (r + 1) * p - 1;" in hip


def test_documents_say_opt_in():
    for name in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "txo_set_guard_beam" in text and "yield" in text, name
