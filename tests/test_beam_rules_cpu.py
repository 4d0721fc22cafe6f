"""No-GPU checks of the constrained beam search (tests/test_gpu_beam_rules.py has the GPU tests): tests/beam_rules_ref.py -- the search in
numpy over a table-driven toy model -- against brute-force enumeration of every sequence, the dead-beam and frozen-state cases on the host,
and what the new switch's Python and C side answer without a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import beam_rules_ref as brr
from texocr_amd import rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, K, EOS = 6, 3, 5


def _toy_rules(depth_max):
    """token 0 opens, 1 closes (need 1), 2 is banned, eos only at depth 0; two states (next = id & 1), state 1 also bans token 3"""
    ids = np.arange(V)
    flags = np.zeros(V, dtype=np.int64)
    flags[2] = R.BAN
    flags[EOS] = R.ONLY_AT_ZERO
    row0 = R.pack(need=(ids == 1).astype(np.int64), delta=(ids == 0).astype(np.int64) - (ids == 1), next=ids & 1, flags=flags)
    f1 = flags.copy()
    f1[3] = R.BAN
    row1 = R.pack(need=(ids == 1).astype(np.int64), delta=(ids == 0).astype(np.int64) - (ids == 1), next=ids & 1, flags=f1)
    return R.TokenRules(np.stack([row0, row1]), depth_max).validate(V)


def _cut(seq, eos):
    seq = list(seq)
    return seq[:seq.index(eos) + 1] if eos in seq else seq


@pytest.mark.parametrize("seed,depth_max,eos_bias", [(0, 1, 0.0), (1, 2, 0.0), (2, 1, 2.0), (3, 2, 3.0)])
def test_search_is_the_brute_force_step_by_step(seed, depth_max, eos_bias):
    """every sequence of length <= 4 over 6 tokens scored on its own (rules.run over the whole sequence, the raw log-probabilities summed):
    a live beam's score is its sequence's, the beams at n + 1 are the k best of ALL sequences that extend a live beam at n, position 1 is
    the k best of all, a beam's state is rules.run of its tokens up to its first eos, and no live beam holds a disallowed token"""
    rng = np.random.RandomState(seed)
    table = rng.randn(V + 1, V) * 1.5
    table[:, EOS] += eos_bias
    rules = _toy_rules(depth_max)
    states = brr.search(table, rules, K, EOS, 4)
    free = brr.search(table, R.TokenRules(np.zeros((1, V), np.int32), 1), K, EOS, 4)
    bound = False
    for n in range(max(states)):
        a, b = states[n], states[n + 1]
        brute = brr.brute_scores(table, rules, EOS, n + 1)
        live_a = {tuple(t) for t, s in zip(a.tokens.tolist(), a.scores) if np.isfinite(s)}
        pool = sorted((s for q, s in brute.items() if q[:n] in live_a and np.isfinite(s)), reverse=True)
        live_b = np.isfinite(b.scores)
        assert int(live_b.sum()) == min(K, len(pool)), n
        np.testing.assert_allclose(b.scores[live_b], pool[:int(live_b.sum())], rtol=0, atol=1e-12)
        if n == 0:
            np.testing.assert_allclose(b.scores[live_b], sorted((s for s in brute.values() if np.isfinite(s)), reverse=True)[:K], atol=1e-12)
        assert bool((b.scores[:-1] >= b.scores[1:]).all())
        for r in np.nonzero(live_b)[0]:
            seq = tuple(b.tokens[r].tolist())
            assert abs(brute[seq] - b.scores[r]) < 1e-12, (n, r)
            st, ok = rules.run(_cut(seq, EOS))
            assert bool(ok.all()) and b.rule_state[r].tolist() == st.tolist(), (n, r)
            assert bool(b.finished[r]) == (EOS in seq)
        bound = bound or (n + 1 in free and not np.array_equal(free[n + 1].tokens, b.tokens))
    assert bound, "the rules never changed a beam: nothing was tested"


def test_allow_all_rules_are_the_plain_search():
    """against tests/beam_ref.py's search64 (the unconstrained definition the GPU replay tests already trust)"""
    import beam_ref as br
    table = np.random.RandomState(5).randn(V + 1, V)
    got = brr.search(table, R.TokenRules(np.zeros((1, V), np.int32), 1), K, EOS, 6)
    want = br.search64(lambda tok: brr.toy_logp(table, tok[0])[None], 1, K, EOS, 6)
    assert max(got) == max(want)
    for n in want:
        assert np.array_equal(got[n].tokens, want[n][0][0]) and np.array_equal(got[n].scores, want[n][1][0]), n
        assert not got[n].rule_state.any()


def test_fewer_allowed_candidates_than_beams():
    """state 0 allows exactly two tokens, state 1 everything, k = 5: two live beams and three dead ones behind position 0, five live from
    position 1 on"""
    table = np.random.RandomState(7).randn(V + 1, V)
    row0 = R.pack(next=np.ones(V, np.int64), flags=np.where(np.isin(np.arange(V), (1, 4)), 0, R.BAN))
    rules = R.TokenRules(np.stack([row0, R.pack(next=np.ones(V, np.int64))]), 1).validate(V)
    states = brr.search(table, rules, 5, None, 3)
    assert np.isfinite(states[1].scores).tolist() == [True, True, False, False, False]
    assert sorted(states[1].tokens[:2, 0].tolist()) == [1, 4]
    for n in (2, 3):
        assert bool(np.isfinite(states[n].scores).all()) and bool(np.isin(states[n].tokens[:, 0], (1, 4)).all())
        assert bool((states[n].rule_state[:, 0] == 1).all())


def test_finished_beams_keep_score_and_state_and_the_search_stops():
    """eos favoured: a finished beam repeats eos at + 0 with its state frozen behind its first eos (the eos advanced it once: next = 1), and
    the search stops at the first position at which every beam is finished or dead"""
    table = np.random.RandomState(9).randn(V + 1, V)
    table[:, EOS] += 6.0
    rules = _toy_rules(2)
    states = brr.search(table, rules, K, EOS, 12)
    last = max(states)
    assert last < 12 and bool((states[last].finished | ~np.isfinite(states[last].scores)).all())
    assert not bool((states[last - 1].finished | ~np.isfinite(states[last - 1].scores)).all())
    seen = 0
    for n in range(1, last):
        a, b = states[n], states[n + 1]
        for r in range(K):
            j = [q for q in range(K) if np.array_equal(a.tokens[q], b.tokens[r, :n])][0]
            if a.finished[j]:
                seen += 1
                assert b.tokens[r, n] == EOS and b.scores[r] == a.scores[j] and b.rule_state[r].tolist() == a.rule_state[j].tolist()
                assert b.rule_state[r].tolist() == [EOS & 1, 0]
    assert seen >= 1


# ---- the switch, where it needs no device ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from texocr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_c_abi_without_gpu(lib):
    from texocr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "texocr.h")).read()
    for name, n_args in (("txo_set_rules_beam", 2), ("txo_last_beam_rule_state", 5)):
        decl = re.search(r"^int " + name + r"\((.*?)\);", hdr, re.M | re.S).group(1)
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        assert len(decl.split(",")) == n_args == len(_lib.SYMBOLS[name][1])
    assert lib.txo_set_rules_beam(None, 1) == _lib.TXO_E_INVALID and "null" in lib.txo_last_error().decode()
    assert lib.txo_last_beam_rule_state(None, None, 1, 1, None) == _lib.TXO_E_INVALID and "null" in lib.txo_last_error().decode()
    fields = [n for n, _ in _lib.TxoBeamOut._fields_]
    assert fields == ["tokens", "scores", "logp", "lengths", "length_alpha"]        # txo_beam_out keeps its layout
    assert C.sizeof(_lib.TxoBeamOut) == 40


def test_python_side_of_the_switch():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from texocr_amd import model, ops, wrapper
    from texocr_amd.config import Dims
    plain, ruled = model.Beams(1, 2, 3, 4), model.Beams(1, 2, 3, 4, 5)
    assert plain.rule_state is None and ruled.rule_state == 5 and ruled.logp == 4
    assert tuple(plain) == tuple(ruled) == (1, 2, 3, 4)           # as a tuple a Beams stays what it was: code that unpacks one keeps working
    for fn in (model.create_model, wrapper.TeXOCRWrapper.__init__):
        assert inspect.signature(fn).parameters["rules_beam"].default is False
    assert isinstance(model.OCRModel.rules_beam, property) and isinstance(model.HipEngine.rules_beam, property)

    class Stub:
        dims, device = Dims(canvas=672), 0
    stub = Stub()                                                 # (the registry keeps a weak reference)
    eid = ops.register_engine(stub)
    try:
        with FakeTensorMode():
            assert torch.ops.texocr.set_rules_beam(eid, True) is None
            st = torch.ops.texocr.last_beam_rule_state(torch.empty((4, 5, 9), dtype=torch.int64), eid)
            assert st.shape == (4, 5, 2) and st.dtype == torch.int32
        with pytest.raises(ValueError, match=r"\(B, beams, n\) GPU tensor"):
            ops.last_beam_rule_state(torch.zeros((2, 3, 4), dtype=torch.int64), eid)
    finally:
        ops.unregister_engine(eid)


def test_documents_say_opt_in():
    for name in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "txo_set_rules_beam" in text and "opt-in" in text, name
