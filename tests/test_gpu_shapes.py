"""The engine's accepted shape space (csrc/engine.hip: validate) against a float64 run of the oracle (tests/ref64.py).

validate() takes any width that is a multiple of 64 in [64, 768], any head count (dim_head is 64, so heads * 64 need not be the width)
and any FFN width that is a multiple of 64; the LayerNorm and decoder-GEMM launches dispatch on the width and on K.  Each case below
is chosen for a branch the rest of the suite never reaches (gpu_harness.SHAPE_CASES).  Small images on a 128x128 canvas keep the encoder cheap:
N = 65, 17, 16 and 2 encoder tokens (128x128, 64x64, 48x80, 16x16), 1, 17 and 2 rows, and in bf16 130 rows of 16x16 images (the
>= 128-row paths).  Per case and storage type:
- encoder rows, the teacher-forced prefix pass (decoder.net: the one-pass prefill where vocab % 8 == 0) and greedy generate with
  logits, against float64;
- where the latent cross attention exists (width 64 / 256 / 768), generate again in latent form;
- fp32: tokens exact up to the first oracle margin < 2e-5, encoder and logits within 1e-4 of float64 (encoder 2e-4 from width 704);
- bf16: max |dlogit| within 1.5x the worse of the two calibration cases (calib256 / calib768, shapes the suite already pins, same depth
  and length), teacher-forced top-1 agreement >= 0.97.  A wrong index gives errors of the order of the logits themselves (~4).
Which path ran is asserted through txo_engine_query, so that a case cannot silently run a different one."""
import numpy as np
import pytest
import torch

import ref64
from gpu_harness import BF16_BOUND, SHAPE_CASES, STOP_ENV, assert_tokens_exact_up_to_margin, build, first_eos, rgb_images
from texocr_amd import synth
from texocr_amd._lib import Q_LAST_COMPACTIONS, Q_LAST_LATENT, Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES

pytestmark = pytest.mark.gpu

STEPS = 24


def _has_latent(d, dtype):
    # lat_attn.h: the tile exists at widths 64 / 256 / 768 where its LDS image fits (la_supported): fp32 at 768 does not
    return d.embed_dim in (64, 256) or (d.embed_dim == 768 and dtype == "bf16")


# (batch, height, width): N = 65, 17, 16, 2 encoder tokens; 17 rows = one 16-row tile and a tail of one
IMAGE_SETS = [(1, 128, 128), (17, 64, 64), (17, 48, 80), (2, 16, 16)]
BF16_ROWS = (130, 16, 16)

_REF = {}


def _ref(case, seed, shape, sd):
    """float64 encoder rows, greedy tokens / step logits and teacher-forced logits of one image set (cached across the dtypes of ONE
    case: the tests run case by case)"""
    key = (case, seed, shape)
    if any(k[0] != case for k in _REF):
        _REF.clear()
    if key not in _REF:
        d = SHAPE_CASES[case][0]
        s64 = ref64.sd64(sd)
        img = rgb_images(*shape, seed)
        enc = ref64.encode(s64, img)
        toks, lg = ref64.generate(s64, enc, d.bos, None, STEPS)
        prefix = torch.cat([torch.full((shape[0], 1), d.bos, dtype=torch.long), toks[:, :-1]], 1)
        tf = ref64.decoder_net(s64, prefix, enc)
        _REF[key] = (img, enc, toks, lg, prefix, tf)
    return _REF[key]


def _expect_persistent(d, dtype, rows):
    # persist_usable (engine.hip): width 256 with 8 heads and FFN factor 4 by default (bf16 up to 128 rows); 768 / 12 heads is opt-in
    return int(d.embed_dim == 256 and d.dec_heads == 8 and d.dec_exp == 4 and (dtype == "fp32" or rows <= 128))


def _expect_ranges(d, dtype, rows, latent):
    # generate (engine.hip): bf16 decodes two row ranges for a wide decoder from 256 rows on, a narrow one beyond 128 (latent form: 224)
    if dtype != "bf16" or rows < 32:
        return 1
    D = d.embed_dim
    want = 2 if (D >= 512 and rows >= 256) or (D < 512 and rows > 128) else 1
    return 1 if (want == 2 and latent and D < 512 and rows < 224) else want


def _agreeing(tok, ref_tok):
    """per row: the steps whose logits were computed from the oracle's own prefix (up to and including the first differing token)"""
    n = tok.shape[1]
    neq = tok != ref_tok
    return np.where(neq.any(1), neq.argmax(1) + 1, n)


def _greedy_err(lg, ref_lg, upto):
    return max(float((lg[b, :u].double() - ref_lg[b, :u]).abs().max()) for b, u in enumerate(upto))


def _sets(dtype):
    return IMAGE_SETS + ([BF16_ROWS] if dtype == "bf16" else [])


def _check_greedy(case, dtype, m, sd, latent, report):
    d = SHAPE_CASES[case][0]
    m.eos_token = None
    for i, shape in enumerate(_sets(dtype)):
        img, enc64, rtok, rlg, prefix, tf64 = _ref(case, 100 + i, shape, sd)
        x = img.cuda()
        tok, lg = m.generate(x, STEPS, return_logits=True)
        got = {q: m._engine.query(q) for q in (Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES, Q_LAST_LATENT)}
        want_p = 0 if latent == 1 else _expect_persistent(d, dtype, shape[0])
        want = {Q_LAST_PERSISTENT: want_p, Q_LAST_ROW_RANGES: 1 if want_p else _expect_ranges(d, dtype, shape[0], latent == 1),
                Q_LAST_LATENT: int(latent == 1)}
        assert got == want, (case, dtype, shape, got, want)
        tok, lg = tok.cpu().numpy(), lg.cpu()
        assert tok.shape == (shape[0], STEPS) and lg.shape == (shape[0], STEPS, d.vocab)
        if dtype == "fp32":
            assert_tokens_exact_up_to_margin(tok, rtok.numpy(), rlg)
        upto = _agreeing(tok, rtok.numpy())
        err = _greedy_err(lg, rlg, upto)
        report.append((f"greedy{'(latent)' if latent == 1 else ''} {shape}", err, float(upto.mean())))
        if dtype == "fp32":
            assert err < 1e-4, (case, shape, err)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", list(SHAPE_CASES))
def test_shape_matrix_against_float64(case, dtype):
    d, what = SHAPE_CASES[case]
    sd = synth.synth_state_dict(d, 3)
    mb = BF16_ROWS[0] if dtype == "bf16" else 17
    latent = 0 if _has_latent(d, dtype) else None
    _, _, m = build(d, sd=sd, dtype=dtype, max_batch=mb, latent=latent)
    report, enc_err, tf_err, same, total = [], 0.0, 0.0, 0, 0
    for i, shape in enumerate(_sets(dtype)):
        img, enc64, rtok, rlg, prefix, tf64 = _ref(case, 100 + i, shape, sd)
        x = img.cuda()
        enc = m.encoder(x)
        assert enc.shape == enc64.shape
        e = float((enc.cpu().double() - enc64).abs().max())
        tf = m.decoder.net(prefix.cuda(), enc=enc).cpu()
        assert tf.shape == tf64.shape
        t = float((tf.double() - tf64).abs().max())
        same, total = same + int((tf.argmax(-1) == tf64.argmax(-1)).sum()), total + tf64.shape[0] * tf64.shape[1]
        report.append((f"encoder / teacher forced {shape}", e, t))
        enc_err, tf_err = max(enc_err, e), max(tf_err, t)
    _check_greedy(case, dtype, m, sd, latent, report)
    agree = same / total
    greedy_err = max(r[1] for r in report if r[0].startswith("greedy"))
    print(f"\n{case} {dtype} ({what}): encoder {enc_err:.2e}, teacher-forced logits {tf_err:.2e}, greedy logits {greedy_err:.2e}, "
          f"teacher-forced top-1 agreement {agree:.4f} of {total}")
    for r in report:
        print("   ", r)
    if dtype == "fp32":
        assert enc_err < (2e-4 if d.embed_dim >= 704 else 1e-4), enc_err
        assert tf_err < 1e-4, tf_err
    else:
        assert enc_err < BF16_BOUND["enc"], enc_err
        assert max(tf_err, greedy_err) < BF16_BOUND["logits"], (tf_err, greedy_err)
        assert agree >= 0.97, agree


@pytest.mark.parametrize("case,dtype", [(c, t) for t in ("fp32", "bf16") for c, (d, _) in SHAPE_CASES.items() if _has_latent(d, t)])
def test_shape_matrix_latent_form(case, dtype):
    """The same greedy decodes with the cross attention in latent form (csrc/lat_attn.h: against the raw encoder rows; TXO_LATENT=1)."""
    d, what = SHAPE_CASES[case]
    sd = synth.synth_state_dict(d, 3)
    mb = BF16_ROWS[0] if dtype == "bf16" else 17
    _, _, m = build(d, sd=sd, dtype=dtype, max_batch=mb, latent=1)
    report = []
    _check_greedy(case, dtype, m, sd, 1, report)
    err = max(r[1] for r in report)
    print(f"\n{case} {dtype} latent form: greedy logits {err:.2e}")
    for r in report:
        print("   ", r)
    if dtype == "bf16":
        assert err < BF16_BOUND["logits"], err


@pytest.mark.parametrize("case", ["w256_h3", "w384_h6", "w768_h20"])
def test_shape_matrix_beam_search_fp32(case):
    """Beam search k = 3 against the oracle's restatement (test_gpu_beam.py: test_beam_search_extension), K/V form and, where it
    exists in fp32, latent form (an image's k beams are ONE row of k * heads heads: 9 at w256_h3).  Beams across several latent tiles:
    test_shape_matrix_beam_search_bf16_latent."""
    d, what = SHAPE_CASES[case]
    sd = synth.synth_state_dict(d, 3)
    s64 = ref64.sd64(sd)
    img = rgb_images(5, 64, 64, 7)
    enc64 = ref64.encode(s64, img)
    ref_t, ref_s = ref64.beam_search(s64, enc64, d.bos, None, STEPS, 3)
    for latent in ((0, 1) if _has_latent(d, "fp32") else (None,)):
        _, _, m = build(d, sd=sd, max_batch=15, latent=latent)
        m.eos_token = None
        toks, scores = m.generate(img.cuda(), STEPS, beam=3, return_beams=True)
        assert m._engine.query(Q_LAST_LATENT) == int(latent == 1)
        err = float((scores.cpu().double() - ref_s).abs().max())
        print(f"\n{case} beam k=3 latent={latent}: max |dscore| {err:.2e}")
        assert torch.equal(toks.cpu(), ref_t), (case, latent)
        assert err < 2e-3, err


# bf16 beams, latent form: max |engine score - float64 score of the same token path| (sums of 24 log-probabilities of about -4 each),
# measured on MI355X: calib768 0.0585, w768_h20 0.0389
BEAM_BF16_CALIB = 0.0585


@pytest.mark.parametrize("case", ["w768_h20", "calib768"])
def test_shape_matrix_beam_search_bf16_latent(case):
    """bf16 beam search k = 3 with the cross attention in latent form: an image's 3 beams are ONE row of 3 * heads heads, 16 to a tile
    (w768_h20: 60 heads, several tiles per row; calib768: 36).  Each returned beam's score against the float64 score of its own token
    path (teacher forced through the oracle): a slot or tile index that mixes beams gives a path whose score is not the engine's.
    Bound: 1.5x calib768's measured error."""
    d, what = SHAPE_CASES[case]
    sd = synth.synth_state_dict(d, 3)
    s64 = ref64.sd64(sd)
    img = rgb_images(5, 64, 64, 7)
    enc64 = ref64.encode(s64, img)
    _, _, m = build(d, sd=sd, dtype="bf16", max_batch=15, latent=1)
    m.eos_token = None
    toks, scores = m.generate(img.cuda(), STEPS, beam=3, return_beams=True)
    assert m._engine.query(Q_LAST_LATENT) == 1
    B, k, n = toks.shape
    assert (B, k, n) == (5, 3, STEPS) and bool((scores[:, :-1] >= scores[:, 1:]).all())
    flat = toks.cpu().reshape(B * k, n)
    prefix = torch.cat([torch.full((B * k, 1), d.bos, dtype=torch.long), flat[:, :-1]], 1)
    lg = ref64.decoder_net(s64, prefix, enc64.repeat_interleave(k, 0))
    path = torch.log_softmax(lg, -1).gather(2, flat[..., None]).sum((1, 2)).view(B, k)
    err = float((scores.cpu().double() - path).abs().max())
    _, ref_s = ref64.beam_search(s64, enc64, d.bos, None, STEPS, k)
    print(f"\n{case} bf16 beam k=3 latent: max |score - float64 path score| {err:.4f}; best beam vs float64 beam search's best "
          f"{float((scores[:, 0].cpu().double() - ref_s[:, 0]).abs().max()):.4f}")
    assert err < 1.5 * BEAM_BF16_CALIB, err


def _stop_sd(d, bias):
    sd = synth.synth_state_dict(d, 3)
    b = sd["decoder.net.to_logits.bias"].copy()
    b[d.eos] += bias
    sd["decoder.net.to_logits.bias"] = b
    return sd


# eos logit bias per case: rows whose first eos falls anywhere over the 24 steps, some never (tuned on the float64 oracle)
STOP_BIAS = {"w192_h3": 2.0, "w768_h20": 2.0}


@pytest.mark.parametrize("case", list(STOP_BIAS))
def test_shape_matrix_row_stop_compaction_fp32(case):
    """stop='row' with a compaction every other position (gpu_harness.py: STOP_ENV): the float64 oracle's tokens bit for bit.  A
    compaction moves a row's K/V history (heads * Tmax * 64 per row): with 3 and 20 heads its stride is not the 8-head one."""
    d, what = SHAPE_CASES[case]
    sd = _stop_sd(d, STOP_BIAS[case])
    img = rgb_images(24, 64, 64, 11) * torch.linspace(0.2, 3.0, 24)[:, None, None, None]
    s64 = ref64.sd64(sd)
    enc64 = ref64.encode(s64, img)
    want, lg = ref64.generate(s64, enc64, d.bos, d.eos, STEPS, stop="row", pad=d.pad)
    first = first_eos(want.numpy(), d.eos)
    assert len(set(first)) >= 6 and -1 in first and min(f for f in first if f >= 0) < 8, first   # the schedule the test is about
    _, _, m = build(d, sd=sd, max_batch=24, latent=0 if _has_latent(d, "fp32") else None, env=STOP_ENV)
    t = m.generate(img.cuda(), STEPS, stop="row")
    assert m._engine.query(Q_LAST_PERSISTENT) == 0 and m._engine.query(Q_LAST_COMPACTIONS) >= 1
    assert np.array_equal(t.cpu().numpy(), want.numpy())
