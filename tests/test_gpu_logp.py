"""GPU tests of generate()'s per-token log-probabilities (txo_generate_logp / txo_generate_from_enc_logp / txo_generate_ragged_logp,
texocr_amd/csrc/step.h + persist.h; OCRModel.generate(return_logp=True)): logp[b, t] = logits[b, t, tok[b, t]] - logsumexp_v
logits[b, t, v], taken from the token selection itself -- no second pass, no (B, T, V) tensor.

References and bounds:
- the float64 oracle (tests/ref64.py), teacher-forced on [bos] + the ENGINE's tokens so that a near-tie cannot make the two runs
  diverge: fp32 within FP32_LOGP = 2e-4 (tests/test_gpu_score.py: the tree's 1e-4 on fp32 logits, doubled for a logit minus a
  log-sum-exp), bf16 within twice gpu_harness.BF16_BOUND["logits"];
- the f32 logits of the SAME call (return_logits=True) through float64 log_softmax: identical operands, so only f32 expf / logf /
  summation error is left -- SAME_LOGITS = 1e-5, derived for |logits| < 16 and V <= 1100: expf and logf about 2 ulp each, the sum of
  at most V/64 + 6 terms (V/64 + 6) * 2^-24 relative, the final subtraction one ulp of a value below 16: under 4e-6 together.  The
  premise |logits| < 16 is asserted, not assumed;
- the engine's other decode paths, the global-stop run, the per-image calls: bit for bit."""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import ref64
from gpu_harness import BF16_BOUND, SHAPE_CASES, STOP_ENV, build, first_eos, knobs, rgb_images, stop_case
from texocr_amd import _lib, synth
from texocr_amd._lib import (Q_LAST_COMPACTIONS, Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES, Q_PERSIST_FALLBACKS, Q_SAMPLE_VOCAB_MAX)
from texocr_amd.config import Dims

pytestmark = pytest.mark.gpu

FP32_LOGP = 2e-4                    # tests/test_gpu_score.py
SAME_LOGITS = 1e-5
W128 = SHAPE_CASES["w128"][0]       # width 128 on a 128x128 canvas, vocabulary 200, 32 positions
TINY_SIZES = [(128, 128), (64, 64), (16, 16), (32, 128), (112, 128), (64, 64), (128, 32)]      # tests/test_gpu_ragged.py


def _vocab(d, vocab, **kw):
    return dataclasses.replace(d, vocab=vocab, bos=vocab - 2, eos=vocab - 3, pad=vocab - 1, **kw)


def _bound(dtype):
    return FP32_LOGP if dtype == "fp32" else 2 * BF16_BOUND["logits"]


def _gather64(logits, toks):
    """float64 log_softmax of logits (B, n, V), gathered at toks (B, n), on the host"""
    return torch.log_softmax(logits.detach().cpu().double(), -1).gather(-1, toks.cpu()[..., None])[..., 0]


def _forced64(sd, d, img, toks):
    """the float64 oracle teacher-forced on [bos] + toks: log_softmax at the tokens (B, n)"""
    s64 = ref64.sd64(sd)
    prefix = torch.cat([torch.full((toks.shape[0], 1), d.bos, dtype=torch.int64), toks.cpu()[:, :-1]], 1)
    return _gather64(ref64.decoder_net(s64, prefix, ref64.encode(s64, img)), toks)


# ---- 1. against float64, token-forced, through every interface -------------------------------------------------------------------
def _c_abi(m, img, n):
    eng = m._engine
    eng._ensure()
    B, Cc, H, W = img.shape
    toks = torch.full((B, n), -7, device="cuda", dtype=torch.int64)
    logp = torch.full((B, n), float("nan"), device="cuda")
    steps = C.c_int32(0)
    _lib.check(eng.lib.txo_generate_logp(eng.handle, img.data_ptr(), B, Cc, H, W, n, -1, toks.data_ptr(), C.byref(steps), None, logp.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert steps.value == n
    return toks, logp


def _custom_op(m, img, n):
    m._engine._ensure()
    toks, steps, logp, logits = torch.ops.texocr.generate_logp(img, m._engine.id, n, -1, False)
    assert int(steps) == n and logits.shape[0] == 0
    return toks, logp


def _module(m, img, n):
    return m.generate(img, n, return_logp=True)


INTERFACES = {"c_abi": _c_abi, "custom_op": _custom_op, "module": _module}


@pytest.mark.parametrize("interface", list(INTERFACES))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_logp_against_float64_token_forced(dtype, interface):
    d, sd, m = build(W128, seed=3, dtype=dtype, max_batch=5)
    m.eos_token = None
    img = rgb_images(5, 48, 80, 900)
    toks, logp = INTERFACES[interface](m, img.cuda(), 16)
    assert toks.shape == (5, 16) and logp.shape == (5, 16) and logp.dtype == torch.float32
    e = float((logp.cpu().double() - _forced64(sd, d, img, toks)).abs().max())
    print(f"logp vs float64 (token-forced), {dtype} via {interface}: max |d| {e:.3e} (bound {_bound(dtype):.1e})")
    assert bool((logp <= 0).all()) and e < _bound(dtype), e


# ---- 2-4. against the logits of the same call, on every branch of the token selection; nothing else moves -------------------------
@pytest.mark.parametrize("decode", ["greedy", "sample"])
@pytest.mark.parametrize("vocab", [200, 203, 1100])
def test_logp_equals_the_log_softmax_of_the_same_calls_logits(vocab, decode):
    """200: V % 4 == 0, one chunk of the arg-max, the register sampler's 16-byte loads; 203: the scalar branches; 1100: two chunks of
    the arg-max (the online rescale across them) and the LDS sampler (beyond the register sampler's 1024 entries)."""
    d = _vocab(W128, vocab)
    d, sd, m = build(d, seed=3, max_batch=7)
    m.eos_token = None
    if vocab > 1024:
        assert m._engine.query(Q_SAMPLE_VOCAB_MAX) >= vocab
    img = rgb_images(7, 48, 80, 910).cuda()
    kw = dict(decode=decode, temp=0.7, seed=5)
    toks, logits, logp = m.generate(img, 14, return_logits=True, return_logp=True, **kw)
    assert toks.shape == (7, 14) and logits.shape == (7, 14, vocab) and logp.shape == (7, 14)
    big = float(logits.abs().max())
    assert big < 16, big                                              # the premise of SAME_LOGITS
    e = float((logp.cpu().double() - _gather64(logits, toks)).abs().max())
    print(f"logp vs log_softmax of the same call's logits, V={vocab} {decode}: max |d| {e:.3e}; max |logit| {big:.2f}")
    assert e < SAME_LOGITS, e
    if decode == "sample":
        assert not torch.equal(toks, logits.argmax(-1)), "sampling never left the arg-max: the sampled logit is not tested"
    # nothing else moves: the same tokens and logits without return_logp, the same tokens and logp without return_logits
    t0, l0 = m.generate(img, 14, return_logits=True, **kw)
    assert torch.equal(t0, toks) and torch.equal(l0, logits)
    assert torch.equal(m.generate(img, 14, **kw), toks)
    t1, p1 = m.generate(img, 14, return_logp=True, **kw)
    assert torch.equal(t1, toks) and torch.equal(p1, logp)


# ---- 5. every decode path gives the same numbers ---------------------------------------------------------------------------------
WIDE = Dims(canvas=64, in_channels=3, embed_dim=256, enc_heads=8, enc_layers=1, dec_heads=8, dec_layers=2, vocab=200, max_len=40,
            bos=198, eos=197, pad=199)              # tests/test_gpu_stop.py: the persistent launch exists for this decoder


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 3, 5, 24, 64, 100, 200])
def test_logp_is_bit_identical_on_every_decode_path(dtype, B):
    """TXO_PERSIST=0 is the baseline; the persistent launch (greedy and sampled kernels), two row ranges and replayed captured steps
    must return its tokens AND its logp bit for bit, and each the tokens it returns without return_logp."""
    d, sd, m = build(WIDE, seed=5, dtype=dtype, max_batch=B, latent=0)  # (beyond 128 rows bf16 launches default to the latent form)
    m.eos_token = None
    eng = m._engine
    g = torch.Generator(device="cuda").manual_seed(40 + B)
    img = torch.rand((B, 3, 32, 64), generator=g, device="cuda")
    modes = {"greedy": dict(), "sample": dict(decode="sample", temp=0.5, seed=9)}
    base = {}
    for name, kw in modes.items():
        with knobs(TXO_PERSIST=0):
            base[name] = m.generate(img, 12, return_logp=True, **kw)
            plain = m.generate(img, 12, **kw)
        assert eng.query(Q_LAST_PERSISTENT) == 0
        assert base[name][1].shape == (B, 12) and torch.equal(base[name][0], plain)
    assert not torch.equal(base["greedy"][0], base["sample"][0])
    for name, kw in modes.items():
        with knobs(TXO_PERSIST=1):
            t, p = m.generate(img, 12, return_logp=True, **kw)
            assert eng.query(Q_LAST_PERSISTENT) == 1 and eng.query(Q_PERSIST_FALLBACKS) == 0, "the persistent launch did not run"
            plain = m.generate(img, 12, **kw)
            assert eng.query(Q_LAST_PERSISTENT) == 1
        assert torch.equal(t, base[name][0]) and torch.equal(plain, t), name
        assert torch.equal(p, base[name][1]), (name, float((p - base[name][1]).abs().max()))
    if B >= 32:
        for name, kw in modes.items():
            with knobs(TXO_LANES=2):
                t, p = m.generate(img, 12, return_logp=True, **kw)
                assert eng.query(Q_LAST_ROW_RANGES) == 2 and eng.query(Q_LAST_PERSISTENT) == 0
                plain = m.generate(img, 12, **kw)
            assert torch.equal(t, base[name][0]) and torch.equal(plain, t) and torch.equal(p, base[name][1]), name
    with knobs(TXO_GRAPH=1):                                          # (a sampled decode never replays captured steps)
        t, p = m.generate(img, 12, return_logp=True)
        assert eng.query(Q_LAST_PERSISTENT) == 0
        plain = m.generate(img, 12)
        t2, p2 = m.generate(img, 12, return_logp=True)               # (again: the step captured by the first call is replayed)
    assert torch.equal(t, base["greedy"][0]) and torch.equal(plain, t) and torch.equal(p, base["greedy"][1])
    assert torch.equal(t2, t) and torch.equal(p2, p)


# ---- 6. per-row stop -------------------------------------------------------------------------------------------------------------
def _check_row_stop(glob, row, eos, pad):
    (tg, pg), (tr, pr) = glob, row
    assert tr.shape == tg.shape and pr.shape == pg.shape
    first = first_eos(tg.cpu().numpy(), eos)
    assert len(set(first)) >= 4 and min(f for f in first if f >= 0) + 1 < tg.shape[1]      # rows finish at different positions
    for b, f in enumerate(first):
        upto = tg.shape[1] if f < 0 else f + 1
        assert torch.equal(tr[b, :upto], tg[b, :upto]), b
        assert torch.equal(pr[b, :upto], pg[b, :upto]), (b, f)                               # bit for bit up to and including the eos
        assert bool((tr[b, upto:] == pad).all())
        assert bool((pr[b, upto:] == 0.0).all()), (b, f, pr[b, upto:])                     # exactly 0.0 behind it
    assert bool(torch.isfinite(pr).all())


@pytest.mark.parametrize("decode", ["greedy", "sample"])
def test_row_stop_logp_follows_the_rows_through_compactions(decode):
    """gpu_harness.stop_case: 40 rows whose first eos falls anywhere, a compaction every other position on two row ranges (greedy:
    replayed captured steps per row count; sampled: eager launches)"""
    d, sd, img = stop_case()
    _, _, m = build(d, sd=sd, max_batch=40, env=STOP_ENV)
    x = img.cuda()
    kw = dict(decode=decode, temp=0.5, seed=123)
    with knobs(TXO_LANES=2):
        glob = m.generate(x, d.max_len, return_logp=True, **kw)
        assert m._engine.query(Q_LAST_COMPACTIONS) == 0
        row = m.generate(x, d.max_len, return_logp=True, stop="row", **kw)
        assert m._engine.query(Q_LAST_COMPACTIONS) > 0 and m._engine.query(Q_LAST_ROW_RANGES) == 2
        plain = m.generate(x, d.max_len, stop="row", **kw)
    assert torch.equal(plain, row[0])
    _check_row_stop(glob, row, d.eos, d.pad)


def test_row_stop_logp_persistent_launch():
    """the persistent launch does not compact: every row keeps decoding and the rewrite behind the decode zeroes logp like it pads"""
    d = WIDE
    sd = synth.synth_state_dict(d, 5)
    b = sd["decoder.net.to_logits.bias"].copy()
    b[d.eos] += 2.5                                                   # tests/test_gpu_stop.py: first eos anywhere in 0..18
    sd["decoder.net.to_logits.bias"] = b
    img = (torch.from_numpy(synth.synth_images(24, 3, 32, 64, seed=3)) * torch.linspace(0.2, 3.0, 24)[:, None, None, None]).cuda()
    _, _, m = build(d, sd=sd, max_batch=24)
    with knobs(TXO_PERSIST=1):
        glob = m.generate(img, d.max_len, return_logp=True)
        row = m.generate(img, d.max_len, return_logp=True, stop="row")
        assert m._engine.query(Q_LAST_PERSISTENT) == 1 and m._engine.query(Q_PERSIST_FALLBACKS) == 0
    _check_row_stop(glob, row, d.eos, d.pad)


# ---- 7. sliding window -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_logp_beyond_the_positional_table(dtype):
    """an 8-position table, 20 tokens: token i >= 8 is picked from the window tokens[i-8 : i] at positions 0..7 (decoder.py:99-100; BOS has
    left it) -- the oracle is forced through the same windows"""
    d = dataclasses.replace(W128, max_len=8)
    d, sd, m = build(d, seed=3, dtype=dtype, max_batch=3)
    m.eos_token = None
    img = rgb_images(3, 48, 80, 920)
    toks, logp = m.generate(img.cuda(), 20, return_logp=True)
    assert toks.shape == (3, 20) and logp.shape == (3, 20)
    assert torch.equal(m.generate(img.cuda(), 20), toks)
    s64 = ref64.sd64(sd)
    enc = ref64.encode(s64, img)
    t = toks.cpu()
    want = torch.empty((3, 20), dtype=torch.float64)
    want[:, :8] = _gather64(ref64.decoder_net(s64, torch.cat([torch.full((3, 1), d.bos, dtype=torch.int64), t[:, :7]], 1), enc), t[:, :8])
    for i in range(8, 20):
        want[:, i] = _gather64(ref64.decoder_net(s64, t[:, i - 8:i].contiguous(), enc)[:, -1:], t[:, i:i + 1])[:, 0]
    err = (logp.cpu().double() - want).abs()
    print(f"sliding window {dtype}: max |dlogp| inside the table {float(err[:, :8].max()):.3e}, beyond it {float(err[:, 8:].max()):.3e}")
    assert float(err.max()) < _bound(dtype), err.max(0).values


# ---- 8. ragged -------------------------------------------------------------------------------------------------------------------
def test_ragged_logp_equals_the_per_image_calls():
    d, sd, m = build(W128, seed=3, max_batch=len(TINY_SIZES))
    m.eos_token = None
    images = [torch.from_numpy(synth.synth_images(1, 3, h, w, seed=200 + i))[0].cuda() for i, (h, w) in enumerate(TINY_SIZES)]
    images[5] = images[1].clone()
    toks, logp = m.generate_ragged(images, 16, return_logp=True)
    assert toks.shape == (7, 16) and logp.shape == (7, 16) and logp.dtype == torch.float32
    assert torch.equal(m.generate_ragged(images, 16), toks)
    for b, im in enumerate(images):
        t1, p1 = m.generate(im[None], 16, return_logp=True)
        n = min(t1.shape[1], toks.shape[1])
        assert torch.equal(toks[b, :n], t1[0, :n]), b
        assert torch.equal(logp[b, :n], p1[0, :n]), (b, TINY_SIZES[b], float((logp[b, :n] - p1[0, :n]).abs().max()))
    assert torch.equal(toks[5], toks[1]) and torch.equal(logp[5], logp[1])


# ---- 9. agreement with score() ---------------------------------------------------------------------------------------------------
def test_logp_agrees_with_scoring_the_generated_tokens():
    """generate's logp against model.score(img, cat([bos], tokens)).logp: two routes through different decoder kernels, each within
    2e-4 of float64 -> 4e-4"""
    d, sd, m = build(W128, seed=3, max_batch=5)
    m.eos_token = None
    img = rgb_images(5, 48, 80, 930).cuda()
    toks, logp = m.generate(img, 16, return_logp=True)
    trg = torch.cat([torch.full((5, 1), d.bos, dtype=torch.int64, device="cuda"), toks], 1)
    s = m.score(img, trg, mask=torch.ones_like(trg, dtype=torch.bool))
    assert bool(s.valid.all())
    e = float((s.logp - logp).abs().max())
    print(f"generate(return_logp) vs score() on the same tokens, fp32: max |d| {e:.3e}")
    assert e < 2 * FP32_LOGP, e


# ---- 10. facades -----------------------------------------------------------------------------------------------------------------
def test_facades_return_logp(tmp_path):
    """TeXOCRWrapper.__call__ / .batch(return_logp=True) on the set-up of tests/test_gpu_ragged.py::test_facades_equal_per_image_calls"""
    from PIL import Image
    from texocr_amd.config import default_config
    from texocr_amd.tokenizer import RegExTokenizer
    from texocr_amd.wrapper import TeXOCRWrapper
    v = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tokenizer_vocab_1k.json")))
    RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"]).save(str(tmp_path / "vocab.txt"))
    cfg = default_config(img_size=[64, 256], max_length=32, in_channels=1,
                         encoder={"embed_dim": 64, "heads": 2, "num_layers": 1}, decoder={"embed_dim": 64, "heads": 2, "num_layers": 2})
    cfg["tokenizer_path"] = str(tmp_path / "vocab.txt")
    w = TeXOCRWrapper(cfg, max_batch=3)
    w.model.load_state_dict(synth.synth_state_dict(w.dims, 5))
    rng = np.random.RandomState(0)
    pil = []
    for wd, ht in [(200, 40), (30, 30), (250, 64), (100, 17), (64, 64), (16, 48), (130, 33)]:
        a = np.full((ht, wd, 3), 255, dtype=np.uint8)
        a[rng.randint(0, ht, 40), rng.randint(0, wd, 40)] = rng.randint(0, 120, (40, 1))
        pil.append(Image.fromarray(a))
    one = [w(im, max_len=20, decode="greedy", return_logp=True) for im in pil]
    got = w.batch(pil, max_len=20, decode="greedy", return_logp=True)
    plain = w.batch(pil, max_len=20, decode="greedy")
    assert len(got) == len(pil) == 7 > w.model._engine.max_batch
    for b, (a, g, p) in enumerate(zip(one, got, plain)):
        assert len(a) == 3 and len(g) == 3 and len(p) == 2
        assert a[0] == g[0] == p[0] and a[1] == g[1] == p[1], b
        assert len(a[2]) == len(a[0]) and len(g[2]) == len(g[0]), b           # cut exactly as the tokens are
        assert a[2] == g[2], (b, a[2], g[2])                                    # batch equals the per-image calls
        assert all(isinstance(x, float) and x <= 0.0 for x in g[2])
    assert w(pil[0], max_len=20, decode="greedy") == one[0][:2]
    x = torch.zeros((1, 1, 32, 32), device="cuda")
    with pytest.raises(ValueError, match="beam search"):
        w.model.generate(x, 8, beam=2, return_logp=True)
