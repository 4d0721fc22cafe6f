"""GPU tests of teacher-forced scoring (txo_decode_score / txo_score, texocr_amd/csrc/score.h, OCRModel.score): per-token
log-probabilities, arg-max and its log-probability of AutoRegressiveDecoder.forward's pass, without a logits buffer.

References: the fixtures tests/golden/score_* captured from the reference (tests/capture_score_golden.py; tests/test_score_cpu.py
pins the CPU oracle to them), the float64 oracle (tests/ref64.py), and the engine's own logits route (decode_prefill -> float64
log_softmax -> gather).  Bounds:
- fp32 logp within 2e-4 of a reference: the tree asserts 1e-4 on fp32 logits (test_gpu_shapes.py) and logp is a logit minus a
  log-sum-exp, which is 1-Lipschitz in the max-norm, so twice that; top1 exact wherever the reference's top-1/top-2 margin >= 2e-5.
- bf16 logp within twice the bound the existing bf16 test of the same shape asserts on logits, top-1 agreement >= 0.97.
- against the engine's own logits route (same operands, another summation order) the bound is twice the measured worst, see
  SAME_OPERANDS_MEASURED below."""
import numpy as np
import pytest
import torch

import ref64
from conftest import load_golden
from gpu_harness import BF16_BOUND, SHAPE_CASES, build, images, oracle, rgb_images
from texocr_amd import _lib, synth
from texocr_amd.config import Dims

pytestmark = pytest.mark.gpu

FP32_LOGP = 2e-4
MARGIN = 2e-5                      # gpu_harness.assert_tokens_exact_up_to_margin's threshold
FIXTURES = ["score_tiny", "score_cfg1", "score_ragged"]

# score vs the logits route of the same session, max |dlogp| over the cases of test_score_equals_the_engines_own_logits_route,
# measured on MI355X (2026-10-16): the two routes multiply the same operands and differ in the order of the f32 sums (and, in
# fp32, in nothing else: both take libm's expf / logf against torch's float64 log_softmax of f32 logits)
SAME_OPERANDS_MEASURED = {"fp32": 1.05e-6, "bf16": 9.8e-7}       # two f32 ulps of a log-probability of about -7


def _fixture(name, dtype="fp32", **kw):
    meta, g = load_golden(name)
    d, sd, m = build(meta, dtype=dtype, **kw)
    trg = torch.from_numpy(g["trg"].astype(np.int64)).cuda()
    mask = torch.from_numpy(g["mask"]).bool().cuda()
    return meta, g, d, sd, m, images(meta).cuda(), trg, mask


def _rand_trg(d, rows, L, seed):
    """bos, then ordinary tokens (never bos / eos / pad)"""
    ordinary = torch.tensor([v for v in range(d.vocab) if v not in (d.bos, d.eos, d.pad)])
    gen = torch.Generator().manual_seed(seed)
    trg = ordinary[torch.randint(0, len(ordinary), (rows, L), generator=gen)]
    trg[:, 0] = d.bos
    return trg


def _from_logits(logits, trg):
    """(logp, top1, top1_logp, margin) of logits (B, L-1, V), in float64 on the host"""
    out = logits.detach().cpu().double()
    lsm = torch.log_softmax(out, -1)
    top1 = out.argmax(-1)
    top2 = out.topk(2, -1).values
    return (lsm.gather(-1, trg.cpu()[:, 1:, None])[..., 0], top1, lsm.gather(-1, top1[..., None])[..., 0], top2[..., 0] - top2[..., 1])


def _c_abi_score(m, img, trg, mask):
    eng = m._engine
    eng._ensure()
    B, Cc, H, W = img.shape
    L = trg.shape[1]
    logp = torch.full((B, L - 1), float("nan"), device="cuda")
    top1 = torch.full((B, L - 1), -7, device="cuda", dtype=torch.int64)
    top1_logp = torch.full((B, L - 1), float("nan"), device="cuda")
    m8 = None if mask is None else mask.to(torch.uint8).contiguous()
    img, trg = img.contiguous(), trg.contiguous()
    _lib.check(eng.lib.txo_score(eng.handle, img.data_ptr(), B, Cc, H, W, trg.data_ptr(), None if m8 is None else m8.data_ptr(), L,
                                 logp.data_ptr(), top1.data_ptr(), top1_logp.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return logp, top1, top1_logp


def _op_score(m, img, trg, mask):
    eng = m._engine
    enc = torch.ops.texocr.encode(img, eng.id)
    torch.ops.texocr.decode_begin(enc, eng.id)
    if mask is not None:
        torch.ops.texocr.decode_set_key_mask(mask[:, :-1].contiguous(), eng.id)
    try:
        return torch.ops.texocr.decode_score(trg, eng.id)
    finally:
        torch.ops.texocr.decode_set_key_mask(None, eng.id)


def _module_score(m, img, trg, mask):
    s = m.score(img, trg)                                  # default mask: trg != trg_pad_idx
    return s.logp, s.top1, s.top1_logp


INTERFACES = {"c_abi": _c_abi_score, "custom_op": _op_score, "module": _module_score}


# ---- 1. fp32 against the reference fixtures, through every interface -------------------------------------------------------------
@pytest.mark.parametrize("interface", list(INTERFACES))
@pytest.mark.parametrize("name", FIXTURES)
def test_fp32_matches_the_reference_fixtures(name, interface):
    meta, g, d, sd, m, img, trg, mask = _fixture(name)
    valid = (mask[:, :-1] & mask[:, 1:]).cpu().numpy()
    logp, top1, top1_logp = (x.cpu().numpy() for x in INTERFACES[interface](m, img, trg, mask if meta["padded"] else None))
    assert logp.shape == g["logp"].shape and top1.shape == g["top1"].shape
    e1, e2 = float(np.abs(logp - g["logp"])[valid].max()), float(np.abs(top1_logp - g["top1_logp"])[valid].max())
    print(f"{name} fp32 via {interface}: max |dlogp| {e1:.2e}, max |dtop1_logp| {e2:.2e} over {int(valid.sum())} valid positions")
    assert e1 < FP32_LOGP and e2 < FP32_LOGP, (e1, e2)
    decided = valid & (g["margin"] >= MARGIN)
    assert np.array_equal(top1[decided], g["top1"].astype(np.int64)[decided])
    if not meta["padded"]:
        s = m.score(img, trg)
        print(f"{name}: loss {float(s.loss):.7f}, the reference's {meta['loss']:.7f}; token_acc {float(s.token_acc):.4f}")
        assert abs(float(s.loss) - meta["loss"]) < FP32_LOGP
        assert bool(s.valid.all()) and s.nll.shape == (trg.shape[0],) and s.loss.ndim == 0
        assert float(s.token_acc) == float((s.top1 == trg[:, 1:]).float().mean())
    else:
        s = m.score(img, trg)
        assert np.array_equal(s.valid.cpu().numpy(), valid)
        want = -(torch.from_numpy(g["logp"]).double() * torch.from_numpy(valid)).sum(1)
        assert float((s.nll.cpu().double() - want).abs().max()) < FP32_LOGP * valid.sum(1).max()
        assert abs(float(s.loss) - float(want.sum() / valid.sum())) < FP32_LOGP


# ---- 2. against the engine's own logits route ------------------------------------------------------------------------------------
def _route_cases(dtype):
    for name in FIXTURES:
        meta, g, d, sd, m, img, trg, mask = _fixture(name, dtype=dtype)
        yield name, m, img, trg, (mask if meta["padded"] else None)
    for case in ("w384_h6", "w768_h20"):
        d = SHAPE_CASES[case][0]
        _, _, m = build(d, seed=3, dtype=dtype, max_batch=6)
        yield case, m, rgb_images(6, 48, 80, 300).cuda(), _rand_trg(d, 6, d.max_len + 1, 301).cuda(), None


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_score_equals_the_engines_own_logits_route(dtype):
    """decode_score against decode_prefill -> float64 log_softmax -> gather on the same session: the same T operands on the same
    MFMA, f32 accumulation in another order.  Measured on MI355X (2026-10-16), max |dlogp| / |dtop1_logp| over the cases here:
    fp32 1.05e-6 (w384_h6), bf16 9.7e-7 (w768_h20) -- two f32 ulps of a log-probability of about -7, in both dtypes, because the
    products are identical and only f32 sums are reordered; no arg-max differs.  Asserted at twice that (the tree's convention for measured bounds)."""
    worst = 0.0
    for name, m, img, trg, mask in _route_cases(dtype):
        eng = m._engine
        enc = m.encoder(img)
        eng.decode_begin(enc)
        if mask is not None:
            eng.set_key_mask(mask[:, :-1])
        logits = eng.decode_prefill(trg[:, :-1].contiguous())
        logp, top1, top1_logp = eng.decode_score(trg)
        eng.set_key_mask(None)
        valid = torch.ones_like(trg[:, 1:], dtype=torch.bool).cpu() if mask is None else (mask[:, :-1] & mask[:, 1:]).cpu()
        r_logp, r_top1, r_top1_logp, margin = _from_logits(logits, trg)
        e = max(float((logp.cpu().double() - r_logp).abs()[valid].max()), float((top1_logp.cpu().double() - r_top1_logp).abs()[valid].max()))
        flips = ((top1.cpu() != r_top1) & valid)
        print(f"score vs logits route, {dtype} {name}: max |dlogp| {e:.3e}; arg-max differs at {int(flips.sum())} of {int(valid.sum())} "
              f"(largest margin among them {float(margin[flips].max()) if flips.any() else 0.0:.2e})")
        assert not bool((flips & (margin >= 2 * max(e, 1e-7))).any())      # a flip needs a margin thinner than twice the deviation
        worst = max(worst, e)
    print(f"score vs logits route, {dtype}: worst {worst:.3e}")
    assert worst <= 2 * SAME_OPERANDS_MEASURED[dtype], worst


# ---- 3. bf16 against the reference and the float64 oracle ------------------------------------------------------------------------
def test_bf16_against_fixture_cfg1():
    """bound: twice the 0.06 that test_gpu_parity.py::test_bf16_mode_logits_error_bounded asserts on this model's bf16 logits"""
    meta, g, d, sd, m, img, trg, mask = _fixture("score_cfg1", dtype="bf16")
    s = m.score(img, trg)
    e = float(np.abs(s.logp.cpu().numpy() - g["logp"]).max())
    agree = float((s.top1.cpu().numpy() == g["top1"]).mean())
    print(f"score_cfg1 bf16 vs reference: max |dlogp| {e:.4f}, top-1 agreement {agree:.4f}, loss {float(s.loss):.5f} vs {meta['loss']:.5f}")
    assert e < 2 * 0.06, e
    assert agree >= 0.97, agree
    assert abs(float(s.loss) - meta["loss"]) < 2 * 0.06


def test_bf16_benchmark_shape_against_float64():
    """64 images of 224 x 672, L = 257 (16384 rows in one chunk).  Bound: twice the 0.038 that
    test_gpu_parity.py::test_bf16_benchmark_shape_vs_reference_every_position asserts on the bf16 logits of this shape."""
    d = Dims(canvas=672)
    d, sd, m = build(d, seed=0, dtype="bf16", max_batch=64, max_tokens=589)
    img = rgb_images(64, 224, 672, 77)
    trg = _rand_trg(d, 64, 257, 78)
    s = m.score(img.cuda(), trg.cuda())
    torch.cuda.synchronize()
    s64 = ref64.sd64(sd)
    r_logp, r_top1, _, _ = _from_logits(ref64.decoder_net(s64, trg[:, :-1], ref64.encode(s64, img)), trg)
    e = float((s.logp.cpu().double() - r_logp).abs().max())
    agree = float((s.top1.cpu() == r_top1).float().mean())
    print(f"benchmark shape bf16 vs float64: max |dlogp| {e:.4f}, top-1 agreement {agree:.4f}")
    assert s.logp.shape == (64, 256)
    assert e < 2 * 0.038, e
    assert agree >= 0.97, agree


# ---- 4. shape matrix against float64 ----------------------------------------------------------------------------------------------
def _oracle_scores(sd, img, trg, mask=None):
    s64 = ref64.sd64(sd)
    enc = ref64.encode(s64, img)
    with torch.no_grad():
        out = oracle().decoder_net(s64, trg.cpu()[:, :-1], enc, mask=None if mask is None else mask.cpu()[:, :-1])
    return _from_logits(out, trg)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["w64_h4", "w192_h3", "w384_h6", "w768_h20"])
def test_shape_matrix_against_float64(case, dtype):
    """widths 64 / 192 / 384 / 768 (1-4 waves per workgroup in score.h), vocabularies 200 / 333 (odd: no logits route exists for
    it) / 1000; L = 2 (one position), L - 1 = 23 (not a multiple of the 16-row block), L = max_len + 1; bf16 w384_h6 at 130 rows."""
    d, _ = SHAPE_CASES[case]
    sd = synth.synth_state_dict(d, 3)
    rows, hw = ((130, (16, 16)) if (dtype, case) == ("bf16", "w384_h6") else (5, (48, 80)))
    _, _, m = build(d, sd=sd, dtype=dtype, max_batch=rows)
    img = rgb_images(rows, *hw, 400)
    enc = m.encoder(img.cuda())
    same = total = 0
    for L in (2, 24, d.max_len + 1):
        trg = _rand_trg(d, rows, L, 401 + L)
        s = m.decoder.score(trg.cuda(), enc=enc)
        assert s.logp.shape == (rows, L - 1) and bool(s.valid.all())
        r_logp, r_top1, r_top1_logp, margin = _oracle_scores(sd, img, trg)
        e = max(float((s.logp.cpu().double() - r_logp).abs().max()), float((s.top1_logp.cpu().double() - r_top1_logp).abs().max()))
        eq = s.top1.cpu() == r_top1
        same, total = same + int(eq.sum()), total + eq.numel()
        print(f"{case} {dtype} L={L}: max |dlogp| vs float64 {e:.3e}, top-1 equal {int(eq.sum())} of {eq.numel()}")
        if dtype == "fp32":
            assert e < FP32_LOGP, (L, e)
            assert bool(eq[margin >= MARGIN].all())
        else:
            assert e < 2 * BF16_BOUND["logits"], (L, e)
        assert bool(((s.top1 >= 0) & (s.top1 < d.vocab)).all())
    if dtype == "bf16":
        assert same / total >= 0.97, same / total


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_odd_vocabulary_equals_the_stepwise_route(dtype):
    """V = 333: txo_decode_prefill cannot give logits (its store epilogue needs V % 8 == 0), scoring must run, and must agree with
    decode_step's logits -> log_softmax.  Bounds: the tree's bound on one-pass vs stepwise logits (test_gpu_parity.py::
    test_prefill_equals_cached_steps_and_continues: 2e-5 in fp32, 0.08 in bf16), doubled for a logit minus a log-sum-exp."""
    d, _ = SHAPE_CASES["w192_h3"]
    assert d.vocab % 8
    _, _, m = build(d, seed=3, dtype=dtype, max_batch=4)
    img = rgb_images(4, 48, 80, 500).cuda()
    trg = _rand_trg(d, 4, 20, 501).cuda()
    enc = m.encoder(img)
    eng = m._engine
    eng.decode_begin(enc)
    with pytest.raises(ValueError):
        eng.decode_prefill(trg[:, :-1].contiguous())                   # existing behaviour: logits_out still refuses
    steps = torch.stack([eng.decode_step(t, trg[:, t].contiguous())[0] for t in range(19)], 1)
    s = m.decoder.score(trg, enc=enc)
    r_logp, r_top1, r_top1_logp, margin = _from_logits(steps, trg)
    e = max(float((s.logp.cpu().double() - r_logp).abs().max()), float((s.top1_logp.cpu().double() - r_top1_logp).abs().max()))
    print(f"odd vocabulary {dtype}: score vs stepwise logits, max |dlogp| {e:.3e}")
    assert e < 2 * (2e-5 if dtype == "fp32" else 0.08), e
    if dtype == "fp32":
        assert bool((s.top1.cpu() == r_top1)[margin >= MARGIN].all())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_image_chunks_when_the_workspace_is_smaller_than_the_block(dtype):
    """max_tokens = 2: the workspace holds 5 x 2 = 10 rows, one image's 7 positions fit, two do not: chunks of ONE image."""
    d, _ = SHAPE_CASES["w64_h4"]
    sd = synth.synth_state_dict(d, 3)
    _, _, m = build(d, sd=sd, dtype=dtype, max_batch=5, max_tokens=2)
    assert (m._engine.max_batch * m._engine.max_tokens) // 7 < 5
    img = rgb_images(5, 16, 16, 600)
    trg = _rand_trg(d, 5, 8, 601)
    s = m.score(img.cuda(), trg.cuda())
    r_logp, r_top1, _, margin = _oracle_scores(sd, img, trg)
    e = float((s.logp.cpu().double() - r_logp).abs().max())
    print(f"image chunks {dtype}: max |dlogp| vs float64 {e:.3e}")
    assert e < (FP32_LOGP if dtype == "fp32" else 2 * BF16_BOUND["logits"]), e
    if dtype == "fp32":
        assert bool((s.top1.cpu() == r_top1)[margin >= MARGIN].all())
    with pytest.raises(ValueError):                                    # a prefix that does not fit the workspace at all
        m.score(img.cuda(), _rand_trg(d, 5, 12, 602).cuda())


# ---- 5. padding ------------------------------------------------------------------------------------------------------------------
def test_padding_rows_do_not_interact_and_padding_content_is_ignored():
    meta, g, d, sd, m, img, trg, mask = _fixture("score_ragged")
    valid = (mask[:, :-1] & mask[:, 1:])
    full = m.score(img, trg)
    assert float((full.logp.cpu() - torch.from_numpy(g["logp"])).abs()[valid.cpu()].max()) < FP32_LOGP
    for b in range(trg.shape[0]):                                      # scored alone: the same bits
        one = m.score(img[b:b + 1], trg[b:b + 1])
        assert torch.equal(one.logp[0][valid[b]], full.logp[b][valid[b]]), b
        assert torch.equal(one.top1[0][valid[b]], full.top1[b][valid[b]]) and torch.equal(one.top1_logp[0][valid[b]], full.top1_logp[b][valid[b]])
        assert float(one.nll[0]) == float(full.nll[b])
    other = torch.where(mask, trg, (trg * 7 + 3) % 60)                  # other tokens BEHIND the padding, the mask given explicitly
    assert not torch.equal(other, trg)
    again = m.score(img, other, mask=mask)
    assert torch.equal(again.logp[valid], full.logp[valid]) and torch.equal(again.top1[valid], full.top1[valid])
    assert torch.equal(again.nll, full.nll) and float(again.loss) == float(full.loss)
    # bf16: valid positions within the bf16 bound of the reference, everything finite
    _, _, mb = build(meta, dtype="bf16")
    sb = mb.score(img, trg)
    eb = float((sb.logp.cpu() - torch.from_numpy(g["logp"])).abs()[valid.cpu()].max())
    print(f"score_ragged bf16 vs reference at valid positions: max |dlogp| {eb:.4f}")
    assert eb < 2 * BF16_BOUND["logits"] and bool(torch.isfinite(sb.logp).all())


# ---- 6. beam scores --------------------------------------------------------------------------------------------------------------
def test_beam_scores_are_the_sum_of_the_scored_log_probabilities():
    """test_gpu_beam.py's case (3 images of 64 x 96, config.yml dims; 4 beams without an eos, 3 beams with one): for every returned
    beam the sum of logp up to and including its first eos is txo_generate_beam's score, within the 2e-3 that test puts on them."""
    d = Dims(canvas=224)
    d, sd, m = build(d, seed=0, max_batch=12)
    img = torch.from_numpy(synth.synth_images(3, 3, 64, 96, seed=41)).cuda()
    m.eos_token = None
    greedy = m.generate(img, 24)
    for k, eos in ((4, None), (3, int(greedy[0, 5]))):
        m.eos_token = eos
        toks, scores = m.generate(img, 24, beam=k, return_beams=True)
        n = toks.shape[2]
        trg = torch.cat([torch.full((3 * k, 1), d.bos, dtype=torch.int64, device="cuda"), toks.reshape(3 * k, n)], 1)
        s = m.score(img.repeat_interleave(k, 0), trg, mask=torch.ones_like(trg, dtype=torch.bool))
        live = torch.ones_like(s.logp, dtype=torch.bool)
        if eos is not None:
            is_eos = (trg[:, 1:] == eos).int()
            live = (torch.cumsum(is_eos, 1) - is_eos) == 0                 # up to and including the first eos
        total = (s.logp.double() * live).sum(1).reshape(3, k)
        err = float((total - scores.double()).abs().max())
        print(f"beam scores vs scored sums (k={k}, eos={eos}, {n} steps): max |d| {err:.2e}")
        assert err < 2e-3, err


# ---- 7. consistency with decoding ------------------------------------------------------------------------------------------------
def test_scoring_a_generated_sequence_and_the_kv_side_effect():
    d = Dims(canvas=224)
    d, sd, m = build(d, seed=5, max_batch=4)
    img = rgb_images(4, 64, 160, 700).cuda()
    m.eos_token = None
    toks, logits = m.generate(img, 24, return_logits=True)
    trg = torch.cat([torch.full((4, 1), d.bos, dtype=torch.int64, device="cuda"), toks], 1)
    s = m.score(img, trg)
    top2 = logits.topk(2, -1).values
    decided = (top2[..., 0] - top2[..., 1]) >= MARGIN
    assert torch.equal(s.top1[decided], toks[decided]) and int(decided.sum()) > 80
    assert float((s.logp - s.top1_logp).abs()[decided].max()) == 0.0    # the target IS the arg-max there
    assert float(s.token_acc) >= float(decided.float().mean())
    # the K/V cache behind decode_score is the one decode_prefill leaves
    eng = m._engine
    enc = m.encoder(img)
    nxt = toks[:, -1].contiguous()
    eng.decode_begin(enc)
    eng.decode_score(trg)
    a, ta = eng.decode_step(24, nxt)
    eng.decode_begin(enc)
    eng.decode_prefill(trg[:, :-1].contiguous(), want_logits=False)
    b, tb = eng.decode_step(24, nxt)
    assert torch.equal(a, b) and torch.equal(ta, tb)
    # run to run: the same bits
    s2 = m.score(img, trg)
    assert torch.equal(s2.logp, s.logp) and torch.equal(s2.top1, s.top1) and torch.equal(s2.top1_logp, s.top1_logp)


# ---- 8. errors -------------------------------------------------------------------------------------------------------------------
def test_errors_and_non_finite_pixels():
    meta, g, d, sd, m, img, trg, mask = _fixture("score_tiny", max_batch=4)
    eng = m._engine
    eng._ensure()
    with pytest.raises(RuntimeError):                                  # no session
        torch.ops.texocr.decode_score(trg, eng.id)
    out = torch.empty((2, 12), device="cuda")
    assert eng.lib.txo_decode_score(eng.handle, trg.data_ptr(), 13, out.data_ptr(), None, None, None) == _lib.TXO_E_STATE
    enc = m.encoder(img)
    with pytest.raises(ValueError):
        m.decoder.score(trg[:, :1], enc=enc)                           # L = 1
    with pytest.raises(ValueError):
        m.decoder.score(_rand_trg(d, 2, d.max_len + 2, 1).cuda(), enc=enc)   # L - 1 > max_len
    with pytest.raises(ValueError):
        m.decoder.score(trg.cpu(), enc=enc)                            # CPU tokens
    with pytest.raises(ValueError):
        m.decoder.score(trg.int(), enc=enc)
    with pytest.raises(ValueError):
        m.decoder.score(trg, mask=mask[:, :-2], enc=enc)
    with pytest.raises(ValueError):
        m.decoder.score(trg, enc=None)
    bad = trg.clone()
    bad[1, 3] = d.vocab
    with pytest.raises(IndexError):
        m.decoder.score(bad, enc=enc)
    eng.decode_begin(enc)
    for L in (1, d.max_len + 2):
        assert eng.lib.txo_decode_score(eng.handle, trg.data_ptr(), L, out.data_ptr(), None, None, None) == _lib.TXO_E_INVALID
    with pytest.raises(NotImplementedError):                           # forward stays the training loss this engine does not implement
        m(img, trg)
    # the C entry point clamps a target outside the table like embed_rows_kernel clamps an input: the clamped id's score
    top = trg.clone()
    top[0, 5] = d.vocab - 1
    eng.decode_begin(enc)
    want = eng.decode_score(top)[0]
    top[0, 5] = d.vocab + 5
    logp = torch.empty((2, 12), device="cuda")
    _lib.check(eng.lib.txo_decode_score(eng.handle, top.data_ptr(), 13, logp.data_ptr(), None, None, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(logp[0, :5], want[0, :5])                        # (position 4 scores target 5; positions from 5 on are FED the clamped id)
    # a non-finite pixel spoils only its own image's scores
    img4 = torch.cat([img, img.flip(0)])
    trg4 = torch.cat([trg, trg.flip(0)])
    clean = m.score(img4, trg4)
    img4[1, 0, 3, 3] = float("nan")
    dirty = m.score(img4, trg4)
    keep = [0, 2, 3]
    assert torch.equal(dirty.logp[keep], clean.logp[keep]) and torch.equal(dirty.top1[keep], clean.top1[keep])
    assert bool(((dirty.top1 >= 0) & (dirty.top1 < d.vocab)).all())
