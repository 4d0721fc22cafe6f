"""GPU tests of the multi-position decoder forward on ragged batches (include/texocr.h: txo_decode_prefill / txo_decode_attn /
txo_decode_score / txo_decode_set_key_mask on a session opened by txo_decode_begin_ragged, txo_score_ragged, the sliding window of
txo_generate_ragged; texocr_amd/csrc/prefill.h and attn_probs.h: RAGGED) and the facades on top: decoder.net / score / align with
n_tokens=, OCRModel.score_ragged / align_ragged, TeXOCRWrapper.batch(return_align=True).

The ragged form is switched on per engine (txo_set_ragged_forward; HipEngine.ragged_forward() around the engine-level calls here, the
facades do it themselves); with the switch off the calls are refused as before, which tests/test_gpu_ragged.py and test 10 here hold.

Two kinds of bound, neither new:
- ragged against the same engine's fixed-shape call on the image alone: exact equality (torch.equal), fp32 and bf16;
- against float64: scores within tests/test_gpu_score.py's FP32_LOGP (2e-4; bf16: 2 * gpu_harness.BF16_BOUND["logits"], what that file
  asserts on bf16 log-probabilities), maps within tests/test_gpu_attn.py's FP32_BOUND (1e-4), rows summing to 1 within keys * EPS."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import attn_ref
import ref64
from gpu_harness import BF16_BOUND, SHAPE_CASES, build
from texocr_amd import _lib, ops, synth
from texocr_amd._lib import Q_LAST_RAGGED
from texocr_amd.config import Dims
from texocr_amd.model import score_summary

pytestmark = pytest.mark.gpu

TINY = SHAPE_CASES["w128"][0]                       # tests/test_gpu_ragged.py: 128x128 canvas, 32 positions, vocabulary 200
TINY_SIZES = [(128, 128), (64, 64), (16, 16), (32, 128), (112, 128), (64, 64), (128, 32)]       # n_b = 65, 17, 2, 17, 57, 17, 17
BENCH = Dims(canvas=224, canvas_w=672)
BENCH_SIZES = [(224, 672), (48, 336), (32, 512), (96, 160)]                                    # n_b = 589, 64, 65, 61
FP32_LOGP = 2e-4                                    # tests/test_gpu_score.py
FP32_MAP, EPS = 1e-4, 2.0 ** -23                    # tests/test_gpu_attn.py: FP32_BOUND, EPS
STEP_VS_PREFILL = 2e-5                              # tests/test_gpu_parity.py::test_prefill_equals_cached_steps_and_continues (fp32)


def _images(sizes, seed, channels=3):
    return [torch.from_numpy(synth.synth_images(1, channels, h, w, seed=seed + i))[0].cuda() for i, (h, w) in enumerate(sizes)]


def _ntok(sizes):
    return [1 + (h // 16) * (w // 16) for h, w in sizes]


def _trg(d, lengths, L, seed):
    """(trg (B, L), mask): bos + ordinary tokens, row b valid over its first lengths[b] columns, pad behind"""
    ordinary = torch.tensor([v for v in range(d.vocab) if v not in (d.bos, d.eos, d.pad)])
    trg = ordinary[torch.randint(0, len(ordinary), (len(lengths), L), generator=torch.Generator().manual_seed(seed))]
    trg[:, 0] = d.bos
    mask = torch.arange(L)[None, :] < torch.tensor(lengths)[:, None]
    trg[~mask] = d.pad
    return trg.cuda(), mask.cuda()


def _solo_scores(m, images, trg, mask):
    rows = [m.score(im[None], trg[b:b + 1], mask[b:b + 1]) for b, im in enumerate(images)]
    return tuple(torch.cat([getattr(r, f) for r in rows]) for f in ("logp", "top1", "top1_logp"))


def _equal_at(valid, got, want, what):
    for g, w, name in zip(got, want, ("logp", "top1", "top1_logp")):
        assert torch.equal(g[valid], w[valid]), f"{what}: {name} of the ragged call is not the solo call's"


def _begun(eng, enc, ntok, passthrough=None):
    """decode_begin_ragged as an expression (for a `with a, b:` line whose second manager needs the session open)"""
    eng.decode_begin_ragged(enc, ntok)
    return passthrough


def _mean_map(eng, x):
    return eng.decode_attn(x, want_logits=False, want_self=False, want_cross=False, want_mean=True)[3]


# ---- 1. score, tiny, fp32 ---------------------------------------------------------------------------------------------------------
def test_score_tiny_fp32():
    d = TINY
    sd = synth.synth_state_dict(d, 3)
    _, _, m = build(d, sd=sd, max_batch=len(TINY_SIZES))
    images = _images(TINY_SIZES, 200)
    L = d.max_len + 1
    trg, mask = _trg(d, [33, 3, 20, 33, 9, 2, 17], L, 11)       # row 0 full length, row 1 two valid targets, row 5 one
    s = m.score_ragged(images, trg)                             # default mask: trg != pad
    valid = mask[:, :-1] & mask[:, 1:]
    assert torch.equal(s.valid, valid) and s.logp.shape == (len(images), L - 1)
    solo = _solo_scores(m, images, trg, mask)
    _equal_at(valid, (s.logp, s.top1, s.top1_logp), solo, "score_ragged")
    # float64 per image on its own encoder rows
    s64 = ref64.sd64(sd)
    worst = 0.0
    for b, im in enumerate(images):
        enc64 = ref64.encode(s64, im[None].cpu(), grid_w=d.grid)
        lsm = torch.log_softmax(ref64.decoder_net(s64, trg[b:b + 1, :-1].cpu(), enc64).double(), -1)
        want = lsm.gather(-1, trg[b:b + 1, 1:, None].cpu())[..., 0]
        worst = max(worst, float((s.logp[b:b + 1].cpu().double() - want).abs()[valid[b:b + 1].cpu()].max()))
    print(f"\n[ragged score fp32 tiny] max |dlogp| vs float64 {worst:.2e} (bound {FP32_LOGP})")
    assert worst < FP32_LOGP
    ref = score_summary(*solo, trg, mask)
    assert torch.equal(s.nll, ref.nll) and torch.equal(s.loss, ref.loss) and torch.equal(s.token_acc, ref.token_acc)
    # the decoder facade over forward_ragged's output, and the C entry point
    enc, ntok = m.encoder.forward_ragged(images)
    s2 = m.decoder.score(trg, mask=mask, enc=enc, n_tokens=ntok)
    _equal_at(valid, (s2.logp, s2.top1, s2.top1_logp), solo, "decoder.score(n_tokens=)")
    eng = m._engine
    box, sizes = ops.pack_ragged(images)
    logp = torch.full((len(images), L - 1), float("nan"), device="cuda")
    top1 = torch.full((len(images), L - 1), -7, device="cuda", dtype=torch.int64)
    top1_logp = torch.full_like(logp, float("nan"))
    m8 = mask.to(torch.uint8).contiguous()
    arr = (C.c_int32 * (2 * len(images)))(*sizes.flatten().tolist())
    with torch.cuda.device(eng.device):
        _lib.check(eng.lib.txo_score_ragged(eng.handle, box.data_ptr(), len(images), 3, box.shape[2], box.shape[3], C.cast(arr, C.POINTER(C.c_int32)),
                                            trg.data_ptr(), m8.data_ptr(), L, logp.data_ptr(), top1.data_ptr(), top1_logp.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    _equal_at(valid, (logp, top1, top1_logp), solo, "txo_score_ragged")


# ---- 2. attention maps, tiny, fp32 --------------------------------------------------------------------------------------------------
def test_attention_maps_tiny_fp32():
    d = TINY
    sd = synth.synth_state_dict(d, 3)
    _, _, m = build(d, sd=sd, max_batch=len(TINY_SIZES))
    eng = m._engine
    images = _images(TINY_SIZES, 200)
    n, B, t = _ntok(TINY_SIZES), len(TINY_SIZES), 9
    Ns = max(n)
    x, mask = _trg(d, [9, 9, 4, 9, 6, 9, 1], t, 12)
    enc, ntok = m.encoder.forward_ragged(images)
    logits, maps = m.decoder.net(x, mask=mask, enc=enc, n_tokens=ntok, return_attn=True)
    assert torch.equal(logits, m.decoder.net(x, mask=mask, enc=enc, n_tokens=ntok)), "return_attn changes the logits"
    assert len(maps) == 2 * d.dec_layers and maps[1].shape == (B, d.dec_heads, t, Ns) and maps[0].shape == (B, d.dec_heads, t, t)
    s64 = attn_ref.sd64(sd)
    worst = 0.0
    for b, im in enumerate(images):
        senc = m.encoder(im[None])
        slog, smaps = m.decoder.net(x[b:b + 1], mask=mask[b:b + 1], enc=senc, return_attn=True)
        v = mask[b]
        assert torch.equal(logits[b][v], slog[0][v]), b
        for i, (got, want) in enumerate(zip(maps, smaps)):
            g = got[b].permute(1, 0, 2)[v]                          # (valid queries, heads, keys)
            w = want[0].permute(1, 0, 2)[v]
            if i % 2:                                               # cross: the image's own keys, exact zeros behind them
                assert torch.equal(g[..., :n[b]], w), (b, i)
                assert bool((got[b][..., n[b]:] == 0).all()), (b, i)
            else:
                assert torch.equal(g, w), (b, i)
            rows = g.double().sum(-1)
            assert float((rows - 1).abs().max()) <= (n[b] if i % 2 else t) * EPS
        _, ref = attn_ref.decoder_attn(s64, x[b:b + 1].cpu(), senc.cpu(), mask[b:b + 1].cpu())
        for i, (got, want) in enumerate(zip(maps, ref)):
            g = got[b].cpu().double().permute(1, 0, 2)[v.cpu()]
            worst = max(worst, float((g[..., :want.shape[-1]] - want[0].permute(1, 0, 2)[v.cpu()]).abs().max()))
    print(f"\n[ragged maps fp32 tiny] max |p - float64| {worst:.2e} (bound {FP32_MAP})")
    assert worst < FP32_MAP
    # buffers the caller filled with NaN: every column behind an image's keys comes back as exactly 0, nothing stays NaN
    Ld, H = d.dec_layers, d.dec_heads
    cp = torch.full((Ld, B, H, t, Ns), float("nan"), device="cuda")
    mean = torch.full((Ld, B, t, Ns), float("nan"), device="cuda")
    with eng.ragged_forward(), eng.key_mask(_begun(eng, enc, ntok, mask)):
        _lib.check(eng.lib.txo_decode_attn(eng.handle, x.data_ptr(), t, None, None, cp.data_ptr(), mean.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(cp).all()) and bool(torch.isfinite(mean).all())
    for b in range(B):
        assert bool((cp[:, b, ..., n[b]:] == 0).all()) and bool((mean[:, b, :, n[b]:] == 0).all()), b
    assert all(torch.equal(cp[l], maps[2 * l + 1]) for l in range(Ld))
    # align_ragged against align per image
    trg, tmask = _trg(d, [10, 10, 5, 10, 7, 10, 2], t + 1, 13)
    for layer in (-1, None):
        al = m.align_ragged(images, trg, tmask, layer=layer)
        assert len(al) == B
        for b, (im, (h, w)) in enumerate(zip(images, TINY_SIZES)):
            solo = m.align(im[None], trg[b:b + 1], tmask[b:b + 1], layer=layer)
            v = tmask[b, :-1]
            assert al[b].maps.shape == (1, t, h // 16, w // 16) == solo.maps.shape
            assert torch.equal(al[b].maps[0][v], solo.maps[0][v]) and torch.equal(al[b].cls[0][v], solo.cls[0][v])
            assert torch.equal(al[b].peak[0][v], solo.peak[0][v])


# ---- 3. stage and block boundaries, benchmark dims ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,t", [("fp32", 5), ("fp32", 130), ("bf16", 5)])
def test_stage_and_block_boundaries_benchmark_dims(dtype, t):
    """n_b = 589 (ten stages, above EA_QBLK), 64 / 65 around EA_KSTAGE, 61; t = 130 is a second query block"""
    d = BENCH
    sd = synth.synth_state_dict(d, 3)
    _, _, m = build(d, sd=sd, dtype=dtype, max_batch=len(BENCH_SIZES))
    eng = m._engine
    images = _images(BENCH_SIZES, 300)
    n = _ntok(BENCH_SIZES)
    trg, mask = _trg(d, [t + 1] * 4, t + 1, 20 + t)
    s = m.score_ragged(images, trg, mask)
    solo = _solo_scores(m, images, trg, mask)
    valid = mask[:, :-1] & mask[:, 1:]
    _equal_at(valid, (s.logp, s.top1, s.top1_logp), solo, f"{dtype} t={t}")
    enc, ntok = m.encoder.forward_ragged(images)
    with eng.ragged_forward():
        eng.decode_begin_ragged(enc, ntok)
        mean = _mean_map(eng, trg[:, :-1].contiguous())
    for b, im in enumerate(images):
        eng.decode_begin(m.encoder(im[None]))
        want = _mean_map(eng, trg[b:b + 1, :-1].contiguous())
        assert torch.equal(mean[:, b:b + 1, :, :n[b]], want), (b, n[b])
        assert bool((mean[:, b, :, n[b]:] == 0).all())
    if t == 5:                                                     # float64 on the image's own float64 encoder rows
        s64 = ref64.sd64(sd)
        worst = 0.0
        for b, im in enumerate(images):
            enc64 = ref64.encode(s64, im[None].cpu(), grid_w=d.grid)
            lsm = torch.log_softmax(ref64.decoder_net(s64, trg[b:b + 1, :-1].cpu(), enc64).double(), -1)
            want = lsm.gather(-1, trg[b:b + 1, 1:, None].cpu())[..., 0]
            worst = max(worst, float((s.logp[b:b + 1].cpu().double() - want).abs().max()))
        bound = FP32_LOGP if dtype == "fp32" else 2 * BF16_BOUND["logits"]      # tests/test_gpu_score.py asserts these on logp
        print(f"\n[ragged score {dtype} benchmark dims] max |dlogp| vs float64 {worst:.2e} (bound {bound})")
        assert worst < bound


# ---- 4. padding is never read ---------------------------------------------------------------------------------------------------------
def test_padding_rows_are_never_read():
    d = TINY
    _, _, m = build(d, seed=3, max_batch=len(TINY_SIZES))
    eng = m._engine
    images = _images(TINY_SIZES, 200)
    n = _ntok(TINY_SIZES)
    enc, ntok = m.encoder.forward_ragged(images)
    trg, mask = _trg(d, [10] * len(images), 10, 14)

    def run(e):
        with eng.ragged_forward():
            eng.decode_begin_ragged(e, ntok)
            sc = eng.decode_score(trg)
            eng.decode_begin_ragged(e, ntok)
            return (*sc, _mean_map(eng, trg[:, :-1].contiguous()))

    base = run(enc)
    assert all(bool(torch.isfinite(o).all()) for o in (base[0], base[2], base[3]))
    for value in (float("nan"), 1e30):
        dirty = enc.clone()
        for b, nb in enumerate(n):
            dirty[b, nb:] = value
        for a, g, name in zip(base, run(dirty), ("logp", "top1", "top1_logp", "cross_mean")):
            assert torch.equal(a, g), f"{name} changed with {value} in the padding rows"
    bad = enc.clone()
    bad[4, 20, 7] = float("nan")                                   # inside image 4's 57 valid rows
    got = run(bad)
    others = [b for b in range(len(images)) if b != 4]
    for a, g in zip(base[:3], got[:3]):
        assert torch.equal(a[others], g[others])
    assert torch.equal(base[3][:, others], got[3][:, others])
    assert not bool(torch.isfinite(got[0][4]).all())


# ---- 5. chunked prefill ---------------------------------------------------------------------------------------------------------------
def test_chunked_prefill_moves_the_key_counts():
    """max_batch * max_tokens = 85 rows, t = 32: chunks of 2, 2, 1 images; key counts 17, 2, 10, 5, 17 differ across the chunks"""
    d = TINY
    sizes = [(64, 64), (16, 16), (48, 48), (32, 32), (128, 32)]
    _, _, m = build(d, seed=3, max_batch=5, max_tokens=17)
    eng = m._engine
    assert (eng.max_batch * eng.max_tokens) // d.max_len == 2
    images = _images(sizes, 210)
    n = _ntok(sizes)
    trg, mask = _trg(d, [33, 12, 33, 20, 33], d.max_len + 1, 15)
    s = m.score_ragged(images, trg, mask)
    _equal_at(mask[:, :-1] & mask[:, 1:], (s.logp, s.top1, s.top1_logp), _solo_scores(m, images, trg, mask), "chunked")
    enc, ntok = m.encoder.forward_ragged(images)
    with eng.ragged_forward():
        eng.decode_begin_ragged(enc, ntok)
        mean = _mean_map(eng, trg[:, :-1].contiguous())
    for b, im in enumerate(images):
        eng.decode_begin(m.encoder(im[None]))
        assert torch.equal(mean[:, b:b + 1, :, :n[b]], _mean_map(eng, trg[b:b + 1, :-1].contiguous())), b
        assert bool((mean[:, b, :, n[b]:] == 0).all())


# ---- 6. continue behind a ragged prefill --------------------------------------------------------------------------------------------
def test_step_continues_behind_a_ragged_prefill():
    """bound: tests/test_gpu_parity.py::test_prefill_equals_cached_steps_and_continues (fp32: 2e-5)"""
    d = TINY
    _, _, m = build(d, seed=3, max_batch=len(TINY_SIZES))
    eng = m._engine
    enc, ntok = m.encoder.forward_ragged(_images(TINY_SIZES, 200))
    x, _ = _trg(d, [6] * len(TINY_SIZES), 6, 16)
    xt = x.t().contiguous()
    eng.decode_begin_ragged(enc, ntok)
    for p in range(5):
        eng.decode_step(p, xt[p], want_logits=False)
    steps = eng.decode_step(5, xt[5])[0].clone()
    with eng.ragged_forward():
        eng.decode_begin_ragged(enc, ntok)
        eng.decode_prefill(x[:, :5].contiguous(), want_logits=False)
    behind = eng.decode_step(5, xt[5])[0]                          # (a step needs no switch)
    err = float((behind - steps).abs().max())
    print(f"\n[ragged prefill, then a step] max |dlogit| vs six steps {err:.2e} (bound {STEP_VS_PREFILL})")
    assert err < STEP_VS_PREFILL


# ---- 7. key mask on a ragged session -------------------------------------------------------------------------------------------------
def test_left_padded_key_mask_on_a_ragged_session():
    d = TINY
    _, _, m = build(d, seed=3, max_batch=4)
    sizes = [(128, 128), (16, 16), (32, 128), (64, 64)]
    images = _images(sizes, 220)
    t = 12
    x, right = _trg(d, [12, 7, 3, 9], t, 17)
    mask = right.flip(1)                                           # left padding: the valid positions are the last ones
    x = torch.where(mask, x.flip(1), torch.full_like(x, d.pad))
    enc, ntok = m.encoder.forward_ragged(images)
    logits, maps = m.decoder.net(x, mask=mask, enc=enc, n_tokens=ntok, return_attn=True)
    for b, im in enumerate(images):
        solo = m.decoder.net(x[b:b + 1], mask=mask[b:b + 1], enc=m.encoder(im[None]))
        assert torch.equal(logits[b][mask[b]], solo[0][mask[b]]), b
        dead = mask[b][:, None] & ~mask[b][None, :]                # query that is not padding, key that is
        for sp in maps[0::2]:
            assert bool((sp[b][:, dead] == 0).all()), b
    # a single step under the mask on the ragged session equals the solo session's
    eng = m._engine
    xt = x.t().contiguous()
    with eng.ragged_forward(), eng.key_mask(_begun(eng, enc, ntok, mask)):
        for p in range(t - 1):
            eng.decode_step(p, xt[p], want_logits=False)
        got = eng.decode_step(t - 1, xt[t - 1])[0].clone()
    for b, im in enumerate(images):
        if bool(mask[b].all()):                                    # (no mask on the solo session: its steps take the fused self-attention launch)
            continue
        eng.decode_begin(m.encoder(im[None]))
        with eng.key_mask(mask[b:b + 1]) as on:
            for p in range(t - 1):
                eng.decode_step(p, xt[p, b:b + 1].contiguous(), want_logits=False)
            assert torch.equal(got[b:b + 1], eng.decode_step(t - 1, xt[t - 1, b:b + 1].contiguous())[0]), (b, on)


# ---- 8. sliding window ------------------------------------------------------------------------------------------------------------------
def test_sliding_window_beyond_the_positional_table():
    d = TINY
    _, _, m = build(d, seed=3, max_batch=4)
    m.eos_token = None
    eng = m._engine
    images = _images([(128, 128), (16, 16), (32, 128), (112, 128)], 230)
    toks = m.generate_ragged(images, 40)
    assert toks.shape == (4, 40) and eng.query(Q_LAST_RAGGED) == 1
    t2, logp = m.generate_ragged(images, 40, return_logp=True)
    assert torch.equal(t2, toks)
    for b, im in enumerate(images):
        st, sl = m.generate(im[None], 40, return_logp=True)
        assert torch.equal(toks[b:b + 1], m.generate(im[None], 40)) and torch.equal(toks[b:b + 1], st), b
        assert torch.equal(logp[b:b + 1], sl), b
    # an engine whose workspace cannot hold one window refuses before it decodes anything
    _, _, small = build(d, seed=3, max_batch=1, max_tokens=17)
    assert small._engine.max_batch * small._engine.max_tokens < d.max_len
    small._engine._ensure()
    box, sizes = ops.pack_ragged([images[1]])
    out = torch.full((1, 40), -7, dtype=torch.int64, device="cuda")
    n = C.c_int32(0)
    arr = (C.c_int32 * 2)(*sizes.flatten().tolist())
    e = small._engine
    with torch.cuda.device(e.device), e.ragged_forward():
        rc = e.lib.txo_generate_ragged(e.handle, box.data_ptr(), 1, 3, 16, 16, C.cast(arr, C.POINTER(C.c_int32)), 40, -1, out.data_ptr(), C.byref(n), None)
    msg = e.lib.txo_last_error().decode()
    torch.cuda.synchronize()
    assert rc == _lib.TXO_E_INVALID and "ragged" in msg and "max_len" in msg and "max_batch * max_tokens" in msg, msg
    assert bool((out == -7).all())
    with pytest.raises(ValueError, match="ragged"):
        small.generate_ragged([images[1]], 40)
    assert small.generate_ragged([images[1]], d.max_len).shape == (1, d.max_len)


# ---- 9. wrapper -------------------------------------------------------------------------------------------------------------------------
def test_wrapper_batch_return_align(tmp_path):
    """the set-up of tests/test_gpu_ragged.py::test_facades_equal_per_image_calls / tests/test_gpu_attn.py::test_wrapper_return_align"""
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
    pil, dims = [], [(200, 40), (30, 30), (130, 33)]
    for wd, ht in dims:
        a = np.full((ht, wd, 3), 255, dtype=np.uint8)
        a[rng.randint(0, ht, 40), rng.randint(0, wd, 40)] = rng.randint(0, 120, (40, 1))
        pil.append(Image.fromarray(a))
    plain = w.batch(pil, max_len=20, decode="greedy")
    got = w.batch(pil, max_len=20, decode="greedy", return_align=True)
    both = w.batch(pil, max_len=20, decode="greedy", return_logp=True, return_align=True)
    for i, (im, (wd, ht)) in enumerate(zip(pil, dims)):
        toks, latex, maps = w(im, max_len=20, decode="greedy", return_align=True)
        assert got[i][0] == toks and got[i][1] == latex and plain[i] == (toks, latex) and len(plain[i]) == 2
        assert got[i][2].shape == (len(toks), -(-ht // 16), -(-wd // 16)) and not got[i][2].is_cuda
        assert torch.equal(got[i][2], maps), i
        assert len(both[i]) == 4 and both[i][:2] == (toks, latex) and torch.equal(both[i][3], maps)


# ---- 10. nothing else moved -------------------------------------------------------------------------------------------------------------
def test_fixed_shape_calls_are_untouched_and_refusals_stay():
    d = TINY
    _, _, m = build(d, seed=3, max_batch=4)
    m.eos_token = None
    eng = m._engine
    x = torch.from_numpy(synth.synth_images(3, 3, 48, 80, seed=9)).cuda()
    trg, mask = _trg(d, [10, 6, 10], 10, 18)

    def fixed():
        s = m.score(x, trg, mask)
        a = m.align(x, trg, mask)
        lg, maps = m.decoder.net(trg[:, :-1].contiguous(), mask=mask[:, :-1], enc=m.encoder(x), return_attn=True)
        return (s.logp, s.top1, s.top1_logp, a.maps, a.cls, lg, *maps)

    before = fixed()
    images = _images([(32, 32), (48, 96), (16, 64)], 40)
    m.score_ragged(images, trg, mask)
    m.align_ragged(images, trg, mask)
    m.generate_ragged(images, 12)
    assert eng.query(Q_LAST_RAGGED) == 1
    assert all(torch.equal(a, b) for a, b in zip(before, fixed())), "a fixed-shape call changed behind ragged ones"
    m.generate(x, 6)
    assert eng.query(Q_LAST_RAGGED) == 0
    # with the switch off (the default) the engine-level calls on a ragged session answer as they always did, and the session still steps
    enc, ntok = m.encoder.forward_ragged(images)
    eng.decode_begin_ragged(enc, ntok)
    for call in (lambda: eng.decode_prefill(trg), lambda: eng.decode_score(trg), lambda: eng.decode_attn(trg), lambda: eng.set_key_mask(mask)):
        with pytest.raises(ValueError, match="ragged batch"):
            call()
    assert bool(torch.isfinite(eng.decode_step(0, trg[:, 0].contiguous())[0]).all())
    with pytest.raises(ValueError, match="ragged batches: max_len"):
        torch.ops.texocr.generate_ragged(*ops.pack_ragged(images), eng.id, d.max_len + 1, -1)
    with eng.ragged_forward():                                     # ... and inside the switch they run; behind it they are refused again
        eng.decode_begin_ragged(enc, ntok)                         # (the refused generate closed the binding's record of the session)
        assert eng.decode_prefill(trg).shape == (3, 10, d.vocab)
    with pytest.raises(ValueError, match="ragged batch"):
        eng.decode_prefill(trg)
    with pytest.raises(ValueError, match="one entry per row"):
        m.decoder.net(trg, enc=m.encoder.forward_ragged(images)[0], n_tokens=torch.tensor([5, 5], dtype=torch.int32))
    with pytest.raises(ValueError, match="one row per image"):
        m.score_ragged(images, trg[:2])
    # beam search is as it was: one (H, W) per call, inside the positional table
    with pytest.raises(ValueError, match="beam search needs max_len"):
        m.generate(x, d.max_len + 1, beam=2)
    rc = eng.lib.txo_generate_beam(eng.handle, x.data_ptr(), 3, 3, 48, 80, 1, d.max_len + 1, -1, torch.empty((3, 40), dtype=torch.int64, device="cuda").data_ptr(),
                                   None, None, None, None)
    assert rc == _lib.TXO_E_INVALID and "cannot slide the window" in eng.lib.txo_last_error().decode()


@pytest.mark.parametrize("what,env", [("hybrid", None), ("latent", {"TXO_LATENT": "1"})])
def test_hybrid_and_forced_latent_still_refuse(what, env):
    if what == "hybrid":
        d = Dims(canvas=64, canvas_w=128, embed="hybrid", in_channels=1, embed_dim=64, enc_heads=1, enc_layers=1, dec_heads=1, dec_layers=1,
                 vocab=32, max_len=8, bos=30, eos=29, pad=31)
        images = [torch.zeros((1, 32, 64), device="cuda"), torch.zeros((1, 64, 32), device="cuda")]
    else:
        d = Dims(canvas=128, in_channels=3, embed_dim=64, enc_heads=2, enc_layers=2, dec_heads=2, dec_layers=2, vocab=64, max_len=48,
                 bos=62, eos=61, pad=63)
        images = [torch.zeros((3, 32, 64), device="cuda"), torch.zeros((3, 64, 32), device="cuda")]
    _, _, m = build(d, seed=1, max_batch=2, env=env)
    trg = torch.full((2, 4), d.bos, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="ragged batches.*(hybrid|latent)"):
        m.score_ragged(images, trg, torch.ones_like(trg, dtype=torch.bool))
    with pytest.raises(ValueError, match="ragged batches.*(hybrid|latent)"):
        m.align_ragged(images, trg, torch.ones_like(trg, dtype=torch.bool))
    with pytest.raises(ValueError, match="ragged batches.*(hybrid|latent)"):
        m.generate_ragged(images, d.max_len + 2)
