"""The encoder at the token and row counts where its tiles end (tests/encoder_cases.py; tests/test_encoder_cases_cpu.py proves that each
case reaches the branch it is listed for), against a float64 run of the oracle (tests/ref64.py).

A. token counts N = 64 .. 257 around the 128-query block and the 64-key stage of csrc/enc_attn.h, at 3, 5 and 8 encoder heads;
B. row counts M = 128 .. 258 across gemm_plain's switch to the LDS-DMA GEMM (csrc/gemm_pp.h: M >= 256) at widths 128, 384 and 704;
C. the persistent tile walk of gemm_pp.h at K = 512 (18 row panels x 16 column tiles on 256 CUs, bands of 6 / 6 / 4), with one and
   with two row super-blocks.
One encoder layer on a 256 x 2032 canvas, engines with max_tokens = 257.  A batch is a few DISTINCT images placed at several slots; the
float64 reference is computed once per distinct image.  Per case and storage type:
- every copy of an image gives bit-identical encoder rows (image b starts at row b * N: its copies sit at different offsets inside row
  panels, query blocks and XCD slots);
- max |d| against float64 over each image's rows, printed apart for the interior rows, the last key stage, the last query block and the
  last row; fp32 within encoder_cases.fp32_bound (1e-4, 2e-4 from width 704), bf16 within gpu_harness.BF16_BOUND["enc"];
- one teacher-forced pass of a 2-token prefix over the whole batch (the cross K/V projection is the other gemm_plain over B * N rows):
  fp32 within 1e-4, bf16 within BF16_BOUND["logits"];
- A only: with the last patch of an image changed, every row of its encoder output changes (no tolerance: the bf16 bound is wider than
  what one key dropped from 193 or 257 moves a row by).

No fp32 case came near its bound (largest 6.4e-6, w512 at N = 193), so encoder_cases.FP32_REBOUND is empty.
bf16 encoder max |d| against float64 measured on MI355X (bound 0.0299; the B = 1 cases equal their B = 5 image bit for bit):
  N          64      65      127     128     129     193     256     257
  w192_h3    0.0221  0.0172  0.0209  0.0188  0.0191  0.0207  0.0214  0.0203
  w256_h3    0.0167  0.0216  0.0165  0.0179  0.0176  0.0159  0.0184  0.0193
  w512       0.0183  0.0156  0.0168  0.0165  0.0161  0.0169  0.0157  0.0174
  rows M     128 .. 258 (N = 2: one figure, the rows never interact)     255 (N = 17)
  w128       0.0118                                                       0.0122
  w384_h6    0.0189                                                       0.0143
  w704_h11   0.0158                                                       0.0171
  w512, 17 slots of N = 257 (M = 4369): 0.0174; teacher-forced logits over all cases at most 0.0283 (bound 0.0557; fp32 5.9e-6)
"""
import pytest
import torch

import encoder_cases as ec
import ref64
from gpu_harness import BF16_BOUND, build, rgb_images
from texocr_amd import synth

pytestmark = pytest.mark.gpu

_SD = {}      # dims name -> (dims, synth state dict, float64 state dict)
_REF = {}     # (dims name, h, w, distinct) -> (images, float64 encoder rows, prefix, float64 teacher-forced logits); never modified


def _weights(name):
    if name not in _SD:
        _SD.clear()
        _REF.clear()                                             # the tests run dims by dims
        d = ec.dims(name)
        sd = synth.synth_state_dict(d, 3)
        _SD[name] = (d, sd, ref64.sd64(sd))
    return _SD[name]


def _ref(case):
    d, sd, s64 = _weights(case.dims)
    key = (case.dims, case.h, case.w, case.distinct)
    if key not in _REF:
        img = rgb_images(case.distinct, case.h, case.w, 1000 + case.n)
        enc = ref64.encode(s64, img, grid_w=d.grid)
        prefix = torch.tensor([[d.bos, 5 + 7 * i] for i in range(case.distinct)], dtype=torch.long)
        _REF[key] = (img, enc, prefix, ref64.decoder_net(s64, prefix, enc))
    return _REF[key]


def _engine(case, dtype):
    d, sd, _ = _weights(case.dims)
    return build(d, sd=sd, dtype=dtype, max_batch=len(case.slots), max_tokens=ec.MAX_TOKENS, env=dict(case.env))[2]


def _encode_and_check(case, dtype, m):
    """the checks of the module docstring; returns the engine's encoder rows (on the GPU)"""
    d = ec.dims(case.dims)
    img, enc64, prefix, tf64 = _ref(case)
    slots = torch.tensor(case.slots)
    enc = m.encoder(img[slots].cuda())
    assert enc.shape == (len(case.slots), case.n, d.embed_dim)
    # ---- slot independence, bit for bit
    first = {}
    for b, s in enumerate(case.slots):
        if s in first:
            same = torch.equal(enc[b], enc[first[s]])
            if not same:
                rows = (enc[b] != enc[first[s]]).any(1).nonzero().flatten().tolist()
                raise AssertionError(f"{case.id} {dtype}: slot {b} (rows from {b * case.n}) differs from slot {first[s]} of the same image "
                                     f"in {len(rows)} rows: {rows[:8]} .. {rows[-1]}")
        else:
            first[s] = b
    # ---- against float64: the maximum over each image's rows, the edges apart
    got = enc.cpu().double()
    bound = ec.fp32_bound(case.id, d) if dtype == "fp32" else BF16_BOUND["enc"]
    worst, lines = 0.0, []
    for s, b in first.items():
        err = (got[b] - enc64[s]).abs().amax(1)                  # per row
        parts = {k: (float(err[list(r)].max()) if len(r) else 0.0) for k, r in ec.edge_rows(case.n).items()}
        lines.append(f"image {s} (slot {b}): " + ", ".join(f"{k} {v:.3e}" for k, v in parts.items()))
        worst = max(worst, float(err.max()))
    print(f"\n{case.id} {dtype} rows {case.rows}: encoder max |d| {worst:.3e} (bound {bound:.1e})")
    for line in lines:
        print("   ", line)
    assert worst < bound, (case.id, dtype, worst, lines)
    # ---- the cross K/V projection over all B * N rows: one teacher-forced pass
    tf = m.decoder.net(prefix[slots].cuda(), enc=enc).cpu().double()
    assert tf.shape == (len(case.slots), 2, d.vocab)
    terr = float((tf - tf64[slots]).abs().max())
    tbound = 1e-4 if dtype == "fp32" else BF16_BOUND["logits"]
    print(f"    teacher-forced logits max |d| {terr:.3e} (bound {tbound:.1e})")
    assert terr < tbound, (case.id, dtype, terr)
    return enc


def _every_row_sees_the_last_key(case, dtype, m, enc):
    """Image a again with only its LAST patch changed: with one encoder layer a row reaches the others through the attention alone, so
    every row of the encoder output has to change.  A row that stays bit-identical never saw key N - 1 (in bf16 a key dropped from 257
    moves the rows by less than the bf16 bound against float64; this needs no bound)."""
    img = _ref(case)[0][:1].clone()
    img[..., case.h - 16:, case.w - 16:] += 0.5
    enc2 = m.encoder(img.cuda())
    a = case.slots.index(0)
    same = (enc2[0] == enc[a]).all(1).nonzero().flatten().tolist()
    assert not same, f"{case.id} {dtype}: {len(same)} rows do not depend on the last key: {same[:8]} .. {same[-1]}"


def _params(cases):
    return [pytest.param(c, t, id=f"{c.id}-{t}") for c in cases for t in ("fp32", "bf16")]


@pytest.mark.parametrize("case,dtype", _params(ec.A_CASES))
def test_token_counts_at_the_attention_tile_edges(case, dtype):
    m = _engine(case, dtype)
    _every_row_sees_the_last_key(case, dtype, m, _encode_and_check(case, dtype, m))


@pytest.mark.parametrize("case,dtype", _params(ec.B_CASES))
def test_row_counts_across_the_gemm_seam(case, dtype):
    _encode_and_check(case, dtype, _engine(case, dtype))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_persistent_walk_at_width_512(dtype):
    """18 row panels x 16 column tiles at the FFN-in, 288 tiles on 256 CUs in bands of 6 / 6 / 4: against float64, and bit for bit
    against an engine whose walk runs two row super-blocks of 16 and 2 panels (TXO_PP_SB_MB=4; read by the bf16 GEMM only)"""
    enc = _encode_and_check(ec.C_CASE, dtype, _engine(ec.C_CASE, dtype))
    slots = torch.tensor(ec.C_CASE_SB.slots)
    enc_sb = _engine(ec.C_CASE_SB, dtype).encoder(_ref(ec.C_CASE_SB)[0][slots].cuda())
    if not torch.equal(enc_sb, enc):
        rows = (enc_sb != enc).flatten(0, 1).any(1).nonzero().flatten().tolist()
        raise AssertionError(f"{dtype}: two super-blocks change {len(rows)} of {ec.C_CASE.rows} rows: {rows[:8]} .. {rows[-1]}")
