"""Alternatives per token on the GPU (csrc/step_alts.h, the k-best form of csrc/score.h): generate(return_alts=k) and score(alts=k) against
tests/alts_ref.py -- a stable descending sort of the f32 row the kernel read, x - logsumexp(x) in float64.

ids are compared EXACTLY wherever the test holds the very floats the kernel read (scripted rows; a call's own return_logits).  Bounds, none
new: test_gpu_logp.SAME_LOGITS for every generate(), test_gpu_score.FP32_LOGP for score(), gpu_harness.assert_tokens_exact_up_to_margin's
2e-5 margin where the reference sums in another order (score on random weights)."""
import os

import numpy as np
import pytest
import torch

import alts_ref
import logit_scripts as ls
from gpu_harness import STOP_ENV, build, first_eos, knobs, on_path, rgb_images, stop_case
from test_gpu_logit_scripts import ROWS, STEPS, WIDE_ROWS, _Engine
from test_gpu_logp import SAME_LOGITS
from test_gpu_sampler import _dims
from test_gpu_score import FP32_LOGP
from texocr_amd import _lib, rules
from texocr_amd._lib import Q_LAST_ALTS, Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES
from texocr_amd.model import Alts

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = alts_ref.MARGIN


def _check_row_alts(name, a, rows, k, bound=SAME_LOGITS):
    """a: Alts (B, n, k); rows: the f32 logits every (row, position) was picked from, (V,) or (B, n, V) -> worst |dlogp|"""
    assert isinstance(a, Alts) and a.ids.dtype == torch.int32 and a.logp.dtype == torch.float32
    ids, lp = a.ids.cpu().numpy(), a.logp.cpu().numpy().astype(np.float64)
    want_ids, want_lp = alts_ref.alts(rows, k)
    want_ids, want_lp = np.broadcast_to(want_ids, ids.shape), np.broadcast_to(want_lp, lp.shape)
    bad = np.argwhere(ids != want_ids)
    assert bad.size == 0, (f"{name}: {len(bad)} of {ids.size} ids differ; first (row, position, rank) {bad[0].tolist()}: {int(ids[tuple(bad[0])])}, "
                           f"expected {int(want_ids[tuple(bad[0])])}")
    e = float(np.abs(lp - want_lp).max())
    assert e < bound, f"{name}: max |alt_logp - float64| {e:.3e} (bound {bound:.0e})"
    return e


def _check_first_is_the_pick(name, tok, lp, a):
    assert torch.equal(a.ids[..., 0].long(), tok), f"{name}: alt_ids[..., 0] is not the token"
    assert torch.equal(a.logp[..., 0], lp), f"{name}: alt_logp[..., 0] is not the call's logp bit for bit"


# ---- 1. scripted rows ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("V", [63, 65, 1024, 1028, 2052])
def test_scripted_rows(V, dtype):
    """zero head weight, the script in the bias: eager launches (the logits are the script, bit for bit), captured steps, stop='row'; bf16 on
    130 rows over two row ranges"""
    eng = _Engine(V, dtype, WIDE_ROWS if dtype == "bf16" else ROWS)
    x = eng.img[:ROWS]
    worst = 0.0
    for sname, row, idx in alts_ref.scripts(V):
        m = eng.load(row)
        for k in alts_ref.KS:
            name = f"V{V}-{sname} k={k} {dtype}"
            tok, lg, lp, a = m.generate(x, STEPS, return_logits=True, return_logp=True, return_alts=k)
            assert (m._engine.query(Q_LAST_PERSISTENT), m._engine.query(Q_LAST_ALTS)) == (0, k)
            assert a.ids.shape == (ROWS, STEPS, k) and a.logp.shape == (ROWS, STEPS, k)
            eng.assert_logits_are_the_script(name, lg)
            worst = max(worst, _check_row_alts(name + " eager", a, row, k))
            _check_first_is_the_pick(name + " eager", tok, lp, a)
            assert a.ids[0, 0, :min(k, len(idx))].tolist() == idx[:k], name
            with knobs(TXO_GRAPH=1, TXO_PERSIST=0):
                tg, lpg, ag = m.generate(x, STEPS, return_logp=True, return_alts=k)
            _check_row_alts(name + " captured steps", ag, row, k)
            _check_first_is_the_pick(name + " captured steps", tg, lpg, ag)
            assert torch.equal(ag.ids, a.ids) and torch.equal(ag.logp, a.logp)
            m.eos_token = next(v for v in range(V - 3, -1, -1) if v not in idx[:1])      # (an eos the script never picks: stop='row' only changes the loop)
            tr, lpr, ar = m.generate(x, STEPS, stop="row", return_logp=True, return_alts=k)
            m.eos_token = None
            _check_row_alts(name + " stop='row'", ar, row, k)
            _check_first_is_the_pick(name + " stop='row'", tr, lpr, ar)
            if dtype == "bf16":
                with knobs(TXO_LANES=2):
                    tw, lgw, lpw, aw = m.generate(eng.img, STEPS, return_logits=True, return_logp=True, return_alts=k)
                assert (m._engine.query(Q_LAST_PERSISTENT), m._engine.query(Q_LAST_ROW_RANGES)) == (0, 2)
                eng.assert_logits_are_the_script(name + " two row ranges", lgw)
                assert aw.ids.shape == (WIDE_ROWS, STEPS, k)
                _check_row_alts(name + " two row ranges", aw, row, k)
                _check_first_is_the_pick(name + " two row ranges", tw, lpw, aw)
    print(f"\nalts V={V} {dtype}: {len(alts_ref.scripts(V))} scripts x k in {alts_ref.KS}: worst |dlogp| {worst:.3e} (bound {SAME_LOGITS:.0e})")


# ---- 2. the call's own logits, random weights ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(dtype):
        if dtype not in cache:
            c = alts_ref.SCORE_CASE
            d = _dims(c["vocab"])
            cache[dtype] = (d, build(d, seed=c["weight_seed"], dtype=dtype, max_batch=ROWS)[2], rgb_images(c["rows"], *c["image_hw"], c["image_seed"]).cuda())
        return cache[dtype]
    return get


@pytest.mark.parametrize("decode", ["greedy", "sample"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_own_logits_random_weights(models, dtype, decode):
    """at every row and position the ids are the stable argsort of the returned f32 logits, exactly: the kernel read those very floats"""
    d, m, x = models(dtype)
    m.eos_token = None
    kw = dict(decode=decode, temp=0.7, seed=5) if decode == "sample" else {}
    tok, lg, lp, a = m.generate(x, STEPS, return_logits=True, return_logp=True, return_alts=8, **kw)
    e = _check_row_alts(f"{dtype} {decode}", a, lg.cpu().numpy(), 8)
    if decode == "greedy":
        _check_first_is_the_pick(f"{dtype} greedy", tok, lp, a)
    print(f"\nalts own logits {dtype} {decode}: |dlogp| {e:.3e} (bound {SAME_LOGITS:.0e})")


# ---- 3. nothing else moves -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decode", ["greedy", "sample"])
def test_nothing_else_moves(models, decode):
    d, m, x = models("fp32")
    m.eos_token = None
    kw = dict(decode=decode, temp=0.7, seed=11) if decode == "sample" else {}
    before = m.generate(x, STEPS, return_logp=True, **kw)
    path = m._engine.query(Q_LAST_PERSISTENT)
    with knobs(TXO_PERSIST=0):
        t0, l0 = m.generate(x, STEPS, return_logp=True, **kw)
        assert m._engine.query(Q_LAST_ALTS) == 0
        t1, l1, a = m.generate(x, STEPS, return_logp=True, return_alts=4, **kw)
    assert (m._engine.query(Q_LAST_PERSISTENT), m._engine.query(Q_LAST_ALTS)) == (0, 4)
    assert torch.equal(t0, t1) and torch.equal(l0, l1)
    after = m.generate(x, STEPS, return_logp=True, **kw)
    assert (m._engine.query(Q_LAST_PERSISTENT), m._engine.query(Q_LAST_ALTS)) == (path, 0)
    assert torch.equal(after[0], before[0]) and torch.equal(after[1], before[1])
    with pytest.raises(ValueError, match="alternatives"):                       # nothing to read behind a call without them
        m._engine.last_alternatives(after[0])


# ---- 4. raw, not masked --------------------------------------------------------------------------------------------------------------------
def test_raw_not_masked_by_rules(models):
    d, m, x = models("fp32")
    m.eos_token = None
    free = m.generate(x, 1)
    banned = sorted(set(free[:, 0].tolist()))                                    # every row's arg-max at position 0
    tok, lg, a, _ = m.generate(x, STEPS, return_logits=True, return_alts=3, rules=rules.ban(d.vocab, banned))
    assert not np.isin(tok.cpu().numpy(), banned).any()
    assert np.isin(a.ids[:, 0, 0].cpu().numpy(), banned).all() and torch.equal(a.ids[:, 0, 0].long(), free[:, 0])
    _check_row_alts("rules", a, lg.cpu().numpy(), 3)
    assert torch.equal(a.ids[..., 0].long(), lg.argmax(-1))


def test_raw_not_masked_by_the_guard():
    """a scripted row (every position's logits are the script): greedy would repeat the maximum, the (1, 1) guard bans the previous pick, so
    the tokens alternate maximum / runner-up while the alternatives stay the raw row's"""
    eng = _Engine(1024)
    sname, row, idx = alts_ref.scripts(1024)[0]
    m = eng.load(row)
    tok, lg, a = m.generate(eng.img, STEPS, return_logits=True, return_alts=3, repeat_guard=(1, 1))
    eng.assert_logits_are_the_script("guard", lg)
    t = tok.cpu().numpy()
    assert (t[:, 0::2] == idx[0]).all() and (t[:, 1::2] == idx[1]).all()        # the banned id (the previous pick) is never the token
    assert bool((a.ids[..., 0] == idx[0]).all())                                 # ... and still the first alternative, at every position
    _check_row_alts("guard", a, row, 3)


# ---- 5. column mapping ---------------------------------------------------------------------------------------------------------------------
def test_prompted_columns(models):
    d, m, x = models("fp32")
    m.eos_token = None
    plen = [1, 2, 3, 4, 4]
    with knobs(TXO_PERSIST=0):
        tok, lp, a = m.generate(x, STEPS, return_logp=True, return_alts=8)
    prefix = torch.cat([torch.full((ROWS, 1), d.bos, dtype=torch.int64, device=tok.device), tok[:, :3]], 1)
    tp, lpp, plp, ap = m.generate(x, 3, prefix=prefix, prefix_len=plen, return_logp=True, return_alts=8)
    for b, n in enumerate(plen):
        assert torch.equal(tp[b], tok[b, n - 1:n + 2])
        assert torch.equal(ap.ids[b], a.ids[b, n - 1:n + 2]) and torch.equal(ap.logp[b], a.logp[b, n - 1:n + 2]), b


def test_stop_row_pads_behind_eos():
    d, sd, img = stop_case()
    m = build(d, sd=sd, max_batch=40, env=STOP_ENV)[2]
    x = img.cuda()
    with knobs(TXO_PERSIST=0):
        tg, ag = m.generate(x, d.max_len, return_alts=3)
        tr, ar = m.generate(x, d.max_len, stop="row", return_alts=3)
    assert m._engine.query(_lib.Q_LAST_COMPACTIONS) > 0
    n = tr.shape[1]
    assert ar.ids.shape == (40, n, 3)
    fe = first_eos(tr.cpu().numpy(), d.eos)
    assert any(0 <= f < n - 1 for f in fe)
    for b, f in enumerate(fe):
        live = n if f < 0 else f + 1
        assert torch.equal(ar.ids[b, :live], ag.ids[b, :live]) and torch.equal(ar.logp[b, :live], ag.logp[b, :live]), b
        assert bool((ar.ids[b, live:] == d.pad).all()) and not bool(ar.logp[b, live:].any()), b


def test_ragged_rows_equal_solo_calls():
    d = _dims(1000)
    m = build(d, seed=3, max_batch=4)[2]
    m.eos_token = None
    imgs = [rgb_images(1, h, w, 20 + i)[0].cuda() for i, (h, w) in enumerate([(32, 48), (16, 64), (48, 32)])]
    tok, lp, a = m.generate_ragged(imgs, STEPS, return_logp=True, return_alts=8)
    assert m._engine.query(Q_LAST_ALTS) == 8
    for b, im in enumerate(imgs):
        ts, ls_, as_ = m.generate_ragged([im], STEPS, return_logp=True, return_alts=8)
        assert torch.equal(ts[0], tok[b]) and torch.equal(as_.ids[0], a.ids[b]) and torch.equal(as_.logp[0], a.logp[b]), b
    _check_first_is_the_pick("ragged", tok, lp, a)


# ---- 6. score, scripted rows -----------------------------------------------------------------------------------------------------------------
def _score_rows(V):
    out = list(alts_ref.scripts(V))
    for a, b in ls.score_pairs(V):
        s = ls.tie(V, a, b)
        out.append((s.name, s.row, list(s.top)))
    return out


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("V", [63, 64, 65, 129, 1027])
def test_score_scripted_rows(V, dtype):
    eng = _Engine(V, dtype, rows=ROWS)
    L, worst = 6, 0.0
    trg = torch.tensor([[eng.d.bos] + [(7 * b + 3 * p) % (V - 3) for p in range(L - 1)] for b in range(ROWS)], dtype=torch.int64).cuda()
    for sname, row, idx in _score_rows(V):
        m = eng.load(row)
        plain = m.score(eng.img, trg)
        for k in alts_ref.KS:
            name = f"score V{V}-{sname} k={k} {dtype}"
            sc, a = m.score(eng.img, trg, alts=k)
            assert a.ids.shape == (ROWS, L - 1, k)
            worst = max(worst, _check_row_alts(name, a, row, k, FP32_LOGP))
            assert torch.equal(a.ids[..., 0].long(), sc.top1) and torch.equal(a.logp[..., 0], sc.top1_logp), name
            for f in sc._fields:
                assert torch.equal(getattr(sc, f), getattr(plain, f), ) or (f in ("loss", "token_acc") and bool(torch.isnan(getattr(sc, f)))), (name, f)
    print(f"\nscore alts V={V} {dtype}: worst |dlogp| {worst:.3e} (bound {FP32_LOGP:.0e})")


# ---- 7. score, random weights ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_score_random_weights(models, dtype):
    d, m, x = models(dtype)
    trg = alts_ref.score_targets(d.bos, d.vocab).cuda()                          # (tests/test_alts_cpu.py: the oracle alone stays inside the cap on this case)
    sc, a = m.score(x, trg, alts=8)
    plain = m.score(x, trg)
    for f in sc._fields:
        assert torch.equal(getattr(sc, f), getattr(plain, f)), f
    assert torch.equal(a.ids[..., 0].long(), sc.top1) and torch.equal(a.logp[..., 0], sc.top1_logp)
    lg = m.decoder.net(trg[:, :-1], enc=m.encoder(x)).double().cpu().numpy()
    want, keep = alts_ref.ranked_places(lg, 8)
    left = int((~keep).sum())
    print(f"\nscore alts random weights {dtype}: {left} of {keep.size} (row, rank) places inside the {MARGIN:.0e} margin are left out")
    assert left <= 0.01 * keep.size
    ids = a.ids.cpu().numpy()
    assert (ids[keep] == want[keep]).all()
    lse = np.log(np.exp(lg - lg.max(-1, keepdims=True)).sum(-1, keepdims=True)) + lg.max(-1, keepdims=True)
    got_lp = a.logp.cpu().numpy().astype(np.float64)
    ref_lp = np.take_along_axis(lg, ids.astype(np.int64), axis=-1) - lse
    assert float(np.abs(got_lp - ref_lp).max()) < FP32_LOGP                      # (both routes multiply the same operands, in either dtype: test_gpu_score)


# ---- 8. refusals, and the C example ----------------------------------------------------------------------------------------------------------
def test_refusals(models):
    d, m, x = models("fp32")
    m.eos_token = None
    eng = m._engine
    with pytest.raises(ValueError, match=r"alternatives: k is 9"):
        m.generate(x, 3, return_alts=9)
    with pytest.raises(ValueError, match=r"alternatives: k is 9"):
        torch.ops.texocr.set_alternatives(eng.id, 9)
    assert eng.lib.txo_set_alternatives(eng.handle, 9) == _lib.TXO_E_INVALID and b"alternatives" in eng.lib.txo_last_error()
    with pytest.raises(ValueError, match="return_alts is not available with beam"):
        m.generate(x[:1], 3, beam=2, return_alts=2)
    with pytest.raises(ValueError, match="return_alts is not available in beam_search"):
        m.beam_search(x[:1], 2, 3, return_alts=2)
    with eng.modes(alts=2):
        with pytest.raises(ValueError, match="beam search: alternatives are not available"):
            eng.generate_beam(x[:1], 2, 3, None)
    with pytest.raises(ValueError, match="alternatives: max_len exceeds the decoder's max_length"):
        m.generate(x, d.max_len + 8, return_alts=2)
    with pytest.raises(ValueError, match="alts= is not available in score_ragged"):
        m.score_ragged([x[0]], torch.zeros((1, 3), dtype=torch.int64).cuda(), alts=2)
    m.generate(x, 3)
    with pytest.raises(ValueError, match="txo_last_alternatives: the last txo_generate\\* ran without alternatives"):
        torch.ops.texocr.last_alternatives(torch.zeros((ROWS, 3), dtype=torch.int64).cuda(), eng.id, 0)
    assert eng.query(Q_LAST_ALTS) == 0 and getattr(eng, "alts", 0) == 0          # every scope put the knob back


def test_k_beyond_the_vocabulary():
    from texocr_amd.config import Dims
    small = Dims(canvas=64, in_channels=3, embed_dim=64, enc_heads=2, enc_layers=1, dec_heads=2, dec_layers=1, vocab=6, max_len=8, bos=4, eos=3, pad=5)
    m = build(small, seed=1, max_batch=1)[2]
    x = rgb_images(1, 32, 32, 1).cuda()
    with pytest.raises(ValueError, match=r"alternatives: k is 8 and the vocabulary has 6 entries"):
        m.generate(x, 3, return_alts=8)
    with pytest.raises(ValueError, match=r"alternatives: k is 8 and the vocabulary has 6 entries"):
        torch.ops.texocr.set_alternatives(m._engine.id, 8)
    assert m._engine.lib.txo_set_alternatives(m._engine.handle, 8) == _lib.TXO_E_INVALID
    assert b"vocabulary has 6 entries" in m._engine.lib.txo_last_error()


def test_torch_free_c_program(tmp_path):
    """examples/alts_tiny.c: plain C + the HIP runtime API: the alternatives of a greedy decode, a refused k, off again"""
    import subprocess
    import sys
    from texocr_amd import build as b
    exe = b.build_example(verbose=False, name="alts_tiny")
    blob = str(tmp_path / "tiny.bin")
    subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), "examples", "make_tiny_blob.py"), blob], check=True, capture_output=True)
    r = subprocess.run([exe, blob], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "is the token and its log-probability, bit for bit" in r.stdout and "alternatives off: tokens are the first run's" in r.stdout
    assert "k = 9: alternatives: k is 9" in r.stdout and "ran without alternatives" in r.stdout
