"""GPU tests of ragged batches (include/texocr.h: txo_encode_ragged / txo_decode_begin_ragged / txo_generate_ragged): B images of
different sizes in one call, every image computed as if it had been passed on its own.

The reference for image b is always the float64 oracle (tests/ref64.py) run ON IMAGE b ALONE.  Bounds are the ones the fixed-shape
tests assert for the same kernels: fp32 encoder rows and logits within 1e-4 (tests/test_gpu_shapes.py), fp32 tokens exact up to the
first oracle margin below 2e-5 (gpu_harness.assert_tokens_exact_up_to_margin), bf16 within gpu_harness.BF16_BOUND.

On a 128x128 canvas an image has at most 8 x 8 patches, and 63 patches (n_b = 64) need a side of 9: the pair n_b = 64 / 65 around
EA_KSTAGE is therefore part of the 224x672 batch (48x336 = 3 x 21 patches, 32x512 = 2 x 32), and the tiny batch holds 57 and 65."""
import ctypes as C

import numpy as np
import pytest
import torch

import ref64
import sampler_ref as sr
from gpu_harness import BF16_BOUND, SHAPE_CASES, STOP_ENV, assert_tokens_exact_up_to_margin, build, first_eos, knobs
from texocr_amd import _lib, ops, synth
from texocr_amd._lib import Q_LAST_COMPACTIONS, Q_LAST_LATENT, Q_LAST_PERSISTENT, Q_LAST_RAGGED, Q_LAST_ROW_RANGES
from texocr_amd.config import Dims

pytestmark = pytest.mark.gpu

TINY = SHAPE_CASES["w128"][0]                       # width 128 on a 128x128 canvas, 3 channels, vocabulary 200, 32 positions
# slot-filling image, a repeated image in slots 1 and 5, 16x16, wide-flat and tall-thin of equal n_b = 17, and 7 x 8 patches
TINY_SIZES = [(128, 128), (64, 64), (16, 16), (32, 128), (112, 128), (64, 64), (128, 32)]
BENCH = Dims(canvas=224, canvas_w=672)              # the benchmark's model
BENCH_SIZES = [(224, 672), (48, 336), (32, 512), (96, 160)]     # n_b = 589 (> EA_QBLK), 64, 65, 61
# bf16 encoder rows of the benchmark model (FOUR encoder layers) against the reference: the bound the existing bf16 test of this model
# asserts (tests/test_gpu_parity.py: test_bf16_mode_logits_error_bounded, 0.15).  gpu_harness.BF16_BOUND["enc"] (0.0299) is calibrated on
# the shape matrix's ONE-layer encoders and is used for those shapes only; the fixed-shape engine itself sits at 0.033-0.045 here.
BENCH_BF16_ENC_BOUND = 0.15


def _images(sizes, seed, channels=3, repeat=None):
    out = [torch.from_numpy(synth.synth_images(1, channels, h, w, seed=seed + i))[0] for i, (h, w) in enumerate(sizes)]
    for dst, src in (repeat or {}).items():
        out[dst] = out[src].clone()
    return out


def _ntok(sizes):
    return [1 + (h // 16) * (w // 16) for h, w in sizes]


def _enc64(sd, images, grid_w):
    s64 = ref64.sd64(sd)
    return s64, [ref64.encode(s64, im[None], grid_w=grid_w)[0] for im in images]


def _check_encoder(d, sizes, seed, repeat=None, dtype="fp32", bound=1e-4):
    sd = synth.synth_state_dict(d, 3)
    _, _, m = build(d, sd=sd, dtype=dtype, max_batch=len(sizes))
    images = _images(sizes, seed, d.in_channels, repeat)
    _, want = _enc64(sd, images, d.grid)
    dev = [im.cuda() for im in images]
    enc, ntok = m.encoder.forward_ragged(dev)
    n, Ns = _ntok(sizes), max(_ntok(sizes))
    assert ntok.tolist() == n and enc.shape == (len(sizes), Ns, d.embed_dim)
    worst, solo_worst = 0.0, 0.0
    for b, nb in enumerate(n):
        err = float((enc[b, :nb].cpu().double() - want[b]).abs().max())
        solo = m.encoder(dev[b][None])[0]                     # the engine's own fixed-shape encode of the image alone
        sdiff = float((enc[b, :nb] - solo).abs().max())
        print(f"\n[ragged encoder {dtype}] image {b} {sizes[b]} n_b={nb}: max |d| vs float64 {err:.2e}; vs solo txo_encode {sdiff:.2e} "
              f"(bit-identical: {sdiff == 0.0})")
        worst, solo_worst = max(worst, err), max(solo_worst, sdiff)
        assert bool((enc[b, nb:] == 0).all()), f"padding rows of slot {b} are not zero"
        assert err < bound, (b, sizes[b], err)
        # ragged row against the same engine's solo run: measured 0 on MI355X (2026-10-17) in fp32 and in bf16 -> asserted exactly
        assert torch.equal(enc[b, :nb], solo), (b, sizes[b], sdiff)
    for dst, src in (repeat or {}).items():
        assert torch.equal(enc[dst], enc[src]), "two copies of one image in different slots differ"
    return m, dev, enc, worst, solo_worst


def test_encoder_parity_fp32_tiny():
    """test 1, tiny dims: B = 7 on a 128x128 canvas (slot-filling image, 16x16, equal-n_b wide / tall, a repeated image)"""
    _check_encoder(TINY, TINY_SIZES, 200, repeat={5: 1})


def test_encoder_parity_fp32_benchmark_dims():
    """test 1, benchmark dims on 224x672: Ns = 589 above EA_QBLK, images of 64 / 65 / 61 tokens under it"""
    _check_encoder(BENCH, BENCH_SIZES, 300)


def test_encoder_parity_bf16_benchmark_dims():
    """test 7, benchmark dims in bf16 on 224x672: Ns = 589, so the image of 61 tokens leaves whole query blocks and key stages of
    enc_attn_bf16_v2_kernel<., true> behind its length; BENCH_BF16_ENC_BOUND against float64, ragged == solo exactly"""
    _check_encoder(BENCH, BENCH_SIZES, 300, dtype="bf16", bound=BENCH_BF16_ENC_BOUND)


def _fill_outside(box, sizes, value):
    out = torch.full_like(box, value)
    for b, (h, w) in enumerate(sizes.tolist()):
        out[b, :, :h, :w] = box[b, :, :h, :w]
    return out


def test_nothing_outside_the_corner_is_read():
    """test 2: NaN, then 1e30, in every pixel of the container outside the images' corners: encoder rows, generated tokens and step
    logits are bit-identical to the zero-filled run.  A NaN pixel INSIDE image b spoils b only."""
    d = TINY
    _, _, m = build(d, max_batch=len(TINY_SIZES), seed=3)
    m.eos_token = None
    eng = m._engine
    images = [im.cuda() for im in _images(TINY_SIZES, 200, repeat={5: 1})]
    box, sizes = ops.pack_ragged(images)
    ntok = ops.ragged_tokens(sizes)

    def run(container):
        enc = torch.ops.texocr.encode_ragged(container, sizes, eng.id)
        toks, n = torch.ops.texocr.generate_ragged(container, sizes, eng.id, 12, -1)
        toks = toks[:, :int(n.item())]
        eng.decode_begin_ragged(enc, ntok)
        prefix = torch.cat([torch.full((len(images), 1), d.bos, dtype=torch.long, device="cuda"), toks[:, :-1]], 1).t().contiguous()
        logits = torch.stack([eng.decode_step(t, prefix[t])[0] for t in range(prefix.shape[0])], 1)
        return enc, toks, logits

    base = run(box)
    assert bool(torch.isfinite(base[0]).all()) and bool(torch.isfinite(base[2]).all())
    for value in (float("nan"), 1e30):
        got = run(_fill_outside(box, sizes, value))
        for a, b, name in zip(base, got, ("encoder", "tokens", "logits")):
            assert torch.equal(a, b), f"{name} changed with {value} outside the corners"
    bad = box.clone()
    bad[2, 0, 3, 5] = float("nan")                            # inside image 2 (16x16)
    got = run(bad)
    others = [b for b in range(len(images)) if b != 2]
    for a, b, name in zip(base, got, ("encoder", "tokens", "logits")):
        assert torch.equal(a[others], b[others]), f"{name} of another slot changed with a NaN inside image 2"


def test_all_sizes_equal_matches_the_fixed_shape_call():
    """test 3: every image the same size: the ragged call agrees with the fixed-shape call within 1e-4 (fp32); prints whether bit-identical"""
    d = TINY
    _, _, m = build(d, max_batch=5, seed=3)
    m.eos_token = None
    x = torch.from_numpy(synth.synth_images(5, 3, 48, 80, seed=9)).cuda()
    enc = m.encoder(x)
    renc, ntok = m.encoder.forward_ragged(list(x))
    assert renc.shape == enc.shape and ntok.tolist() == [16] * 5
    diff = float((renc - enc).abs().max())
    toks, lg = m.generate(x, 16, return_logits=True)
    rtoks = m.generate_ragged(list(x), 16)
    print(f"\n[ragged == fixed, equal sizes] encoder max |d| {diff:.2e} (bit-identical: {torch.equal(renc, enc)}); "
          f"tokens identical: {torch.equal(toks, rtoks)}")
    assert diff < 1e-4
    ref_lg = lg.cpu().double()
    assert_tokens_exact_up_to_margin(rtoks.cpu().numpy(), toks.cpu().numpy(), ref_lg)


# ---- decode: 40 rows of mixed sizes, eos favoured by a logit bias (the schedule of gpu_harness.stop_case on a 128x128 canvas) ----------
RAG_DIMS = Dims(canvas=128, in_channels=3, embed_dim=64, enc_heads=2, enc_layers=2, dec_heads=2, dec_layers=2, vocab=64, max_len=48,
                bos=62, eos=61, pad=63)
MIX_SIZES = [(32, 48), (128, 128), (16, 16), (64, 96), (32, 128), (128, 32), (48, 48), (112, 128)]
_MIX = {}


def mixed_case(rows=40, bias=1.2):
    """rows images cycling through MIX_SIZES with contrasts 0.2 .. 3.0; per image ALONE in float64: encoder rows, greedy tokens and step
    logits over max_len positions with eos=None, and the first-eos position (-1: none)"""
    if "case" not in _MIX:
        d = RAG_DIMS
        sd = synth.synth_state_dict(d, 7)
        b = sd["decoder.net.to_logits.bias"].copy()
        b[d.eos] += bias
        sd["decoder.net.to_logits.bias"] = b
        sizes = [MIX_SIZES[i % len(MIX_SIZES)] for i in range(rows)]
        scale = torch.linspace(0.2, 3.0, rows)
        images = [im * scale[i] for i, im in enumerate(_images(sizes, 11))]
        s64, enc = _enc64(sd, images, d.grid)
        solo = [ref64.generate(s64, e[None], d.bos, None, d.max_len) for e in enc]
        toks = torch.cat([t for t, _ in solo], 0)
        logits = torch.cat([l for _, l in solo], 0)
        _MIX["case"] = (d, sd, sizes, images, enc, toks, logits, first_eos(toks.numpy(), d.eos))
    return _MIX["case"]


def _expected_steps(first, max_len):
    return max_len if -1 in first else max(first) + 1


def test_decode_teacher_forced_logits_fp32():
    """test 4a: txo_decode_begin_ragged + teacher-forced txo_decode_step: every position's logits within 1e-4 of the oracle per image"""
    d, sd, sizes, images, enc64, rtok, rlg, first = mixed_case()
    _, _, m = build(d, sd=sd, max_batch=len(images))
    eng = m._engine
    enc, ntok = m.encoder.forward_ragged([im.cuda() for im in images])
    eng.decode_begin_ragged(enc, ntok)
    steps = 24
    prefix = torch.cat([torch.full((len(images), 1), d.bos, dtype=torch.long), rtok[:, :steps - 1]], 1).t().contiguous().cuda()
    logits = torch.stack([eng.decode_step(t, prefix[t])[0] for t in range(steps)], 1).cpu().double()
    err = (logits - rlg[:, :steps]).abs().amax(dim=(1, 2))
    print(f"\n[ragged decode fp32] teacher-forced logits, max |d| per image vs float64: worst {float(err.max()):.2e} (image {int(err.argmax())})")
    assert float(err.max()) < 1e-4, err


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("lanes", [1, 2])
def test_generate_ragged_tokens_fp32(lanes, graph):
    """test 4b: generate_ragged with the global eos break, on one and two row ranges, eager and replayed: every row's tokens are the
    oracle's solo tokens (eos=None) over the batch's n_steps = max over rows of the solo first-eos position + 1"""
    d, sd, sizes, images, enc64, rtok, rlg, first = mixed_case()
    _, _, m = build(d, sd=sd, max_batch=len(images))
    with knobs(TXO_LANES=lanes, TXO_GRAPH=graph):
        t = m.generate_ragged([im.cuda() for im in images], d.max_len)
    eng = m._engine
    assert eng.query(Q_LAST_RAGGED) == 1 and eng.query(Q_LAST_PERSISTENT) == 0 and eng.query(Q_LAST_LATENT) == 0
    assert eng.query(Q_LAST_ROW_RANGES) == lanes
    n = _expected_steps(first, d.max_len)
    assert t.shape == (len(images), n), (t.shape, n)
    assert_tokens_exact_up_to_margin(t.cpu().numpy(), rtok[:, :n].numpy(), rlg[:, :n])


@pytest.mark.parametrize("lanes", [1, 2])
def test_per_row_stop_lengths_move_with_rows(lanes):
    """test 5: stop='row' with a compaction every other position: every row equals the oracle's stop='row' result for that image alone
    (its tokens up to its first eos, pad behind).  A length that stayed in its slot would give a moved row another image's key count."""
    d, sd, sizes, images, enc64, rtok, rlg, first = mixed_case()
    # the schedule the test is about: rows that finish at once stand in front of rows of OTHER sizes that finish late or never, so live rows move
    assert min(f for f in first if f >= 0) < 8 and max(first) > 16 and -1 in first and len(set(first)) >= 3, first
    n = _expected_steps(first, d.max_len)
    want = rtok[:, :n].clone()
    for b, f in enumerate(first):
        if f >= 0:
            want[b, f + 1:] = d.pad
    _, _, m = build(d, sd=sd, max_batch=len(images), env=STOP_ENV)
    with knobs(TXO_LANES=lanes):
        t = m.generate_ragged([im.cuda() for im in images], d.max_len, stop="row")
    assert m._engine.query(Q_LAST_COMPACTIONS) > 0 and m._engine.query(Q_LAST_ROW_RANGES) == lanes
    assert t.shape == tuple(want.shape)
    margin = ref64.margins(rlg[:, :n])
    for b in range(len(images)):
        upto = first[b] + 1 if first[b] >= 0 else n
        small = np.nonzero(margin[b, :upto].numpy() < 2e-5)[0]
        assert small.size == 0, "the case must decide every token by more than the fp32 error"
        assert np.array_equal(t[b].cpu().numpy(), want[b].numpy()), (b, sizes[b], first[b])
    # a fixed-shape generate directly behind it starts from scratch
    x = torch.stack([im for im, s in zip(images, sizes) if s == sizes[0]]).cuda()
    a = m.generate(x, 12)
    assert m._engine.query(Q_LAST_RAGGED) == 0 and m._engine.query(Q_LAST_COMPACTIONS) == 0 and a.shape[0] == x.shape[0]


BAND = 2e-5                                         # tests/test_gpu_sampler.py: of the kept mass


def test_sampled_decode_draws_on_the_rows_own_logits():
    """test 6: decode='sample': token i of batch row b is the host sampler's draw (tests/sampler_ref.py) under the key (seed; b, i) on
    the row's own logits (the engine's teacher-forced logits of the ragged session for the sampled prefix)"""
    d, sd, sizes, images, *_ = mixed_case()
    _, _, m = build(d, sd=sd, max_batch=len(images))
    m.eos_token = None
    eng = m._engine
    dev = [im.cuda() for im in images]
    temp, seed, steps = 0.7, 321, 20
    tok = m.generate_ragged(dev, steps, temp=temp, decode="sample", seed=seed)
    assert tok.shape == (len(images), steps)
    enc, ntok = m.encoder.forward_ragged(dev)
    eng.decode_begin_ragged(enc, ntok)
    prefix = torch.cat([torch.full((len(images), 1), d.bos, dtype=torch.long, device="cuda"), tok[:, :-1]], 1).t().contiguous()
    lg = torch.stack([eng.decode_step(t, prefix[t])[0] for t in range(steps)], 1).cpu().numpy()
    B = len(images)
    dr = sr.draw(lg.reshape(-1, d.vocab), temp, seed, np.repeat(np.arange(B), steps), np.tile(np.arange(steps), B))
    got = tok.cpu().numpy().reshape(-1)
    outside = dr.dist > BAND
    assert not (outside & (got != dr.token)).any(), "a draw away from any boundary differs from the host rule"
    assert bool(((got == dr.pair[:, 0]) | (got == dr.pair[:, 1]))[~outside].all())
    assert float((~outside).mean()) < 0.02


@pytest.mark.parametrize("case", ["calib256"])
def test_bf16_calibration_shape(case):
    """test 7: the calibration shape in bf16, mixed sizes: encoder rows and teacher-forced logits against float64 per image within the
    bound the fixed-shape bf16 tests use (gpu_harness.BF16_BOUND), top-1 agreement >= 0.97; ragged rows against the same engine's solo
    encode are printed and asserted at the oracle bound (never looser)."""
    d = SHAPE_CASES[case][0]
    m, dev, enc, worst, solo = _check_encoder(d, TINY_SIZES, 200, repeat={5: 1}, dtype="bf16", bound=BF16_BOUND["enc"])
    print(f"\n[ragged bf16 {case}] encoder vs float64 {worst:.4f} (bound {BF16_BOUND['enc']:.4f}); ragged row vs solo run {solo:.4f}")
    sd = synth.synth_state_dict(d, 3)
    images = _images(TINY_SIZES, 200, repeat={5: 1})
    s64, enc64 = _enc64(sd, images, d.grid)
    steps = 24
    ref = [ref64.generate(s64, e[None], d.bos, None, steps) for e in enc64]
    rtok = torch.cat([t for t, _ in ref], 0)
    prefix = torch.cat([torch.full((len(images), 1), d.bos, dtype=torch.long), rtok[:, :-1]], 1)
    tf64 = torch.cat([ref64.decoder_net(s64, prefix[b:b + 1], enc64[b][None]) for b in range(len(images))], 0)
    eng = m._engine
    eng.decode_begin_ragged(enc, ops.ragged_tokens(torch.tensor(TINY_SIZES, dtype=torch.int32)))
    pt = prefix.t().contiguous().cuda()
    lg = torch.stack([eng.decode_step(t, pt[t])[0] for t in range(steps)], 1).cpu().double()
    err = float((lg - tf64).abs().max())
    agree = float((lg.argmax(-1) == tf64.argmax(-1)).float().mean())
    print(f"[ragged bf16 {case}] teacher-forced logits vs float64 {err:.4f} (bound {BF16_BOUND['logits']:.4f}), top-1 agreement {agree:.4f}")
    assert err < BF16_BOUND["logits"] and agree >= 0.97


def test_bf16_benchmark_shape_130_rows_two_ranges():
    """test 7: the benchmark model in bf16, 130 rows of five sizes on two row ranges.  Every row against the float64 oracle of that image
    alone: encoder rows within BENCH_BF16_ENC_BOUND, teacher-forced step logits (the oracle's tokens fed) within gpu_harness.BF16_BOUND,
    top-1 agreement >= 0.97 (measured on MI355X, 2026-10-17: 0.0449, 0.0452, 0.9846).
    Every row against the same engine's fixed-shape run of that image: encoder rows, and the step logits of a fixed-shape session over
    the images of its size -- measured 0 on MI355X (2026-10-17), asserted exactly."""
    d = BENCH
    sd = synth.synth_state_dict(d, 3)
    kinds = [(32, 64), (16, 16), (64, 96), (48, 160), (224, 32)]
    sizes = [kinds[i % 5] for i in range(130)]
    images = _images(sizes, 500)
    _, _, m = build(d, sd=sd, dtype="bf16", max_batch=130, max_tokens=40)
    m.eos_token = None
    eng = m._engine
    steps = 8
    dev = [im.cuda() for im in images]
    tok = m.generate_ragged(dev, steps).cpu()
    assert eng.query(Q_LAST_ROW_RANGES) == 2 and eng.query(Q_LAST_RAGGED) == 1 and eng.query(Q_LAST_LATENT) == 0
    assert tok.shape == (130, steps)
    s64, enc64 = _enc64(sd, images, d.grid)
    ref = [ref64.generate(s64, e[None], d.bos, None, steps) for e in enc64]
    rtok = torch.cat([t for t, _ in ref], 0)
    rlg = torch.cat([l for _, l in ref], 0)                     # greedy: the oracle's own tokens are its teacher-forced prefix
    enc, ntok = m.encoder.forward_ragged(dev)
    enc_err = max(float((enc[b, :n].cpu().double() - enc64[b]).abs().max()) for b, n in enumerate(ntok.tolist()))
    prefix = torch.cat([torch.full((130, 1), d.bos, dtype=torch.long), rtok[:, :-1]], 1).t().contiguous().cuda()
    eng.decode_begin_ragged(enc, ntok)
    lg = torch.stack([eng.decode_step(t, prefix[t])[0] for t in range(steps)], 1)
    err = float((lg.cpu().double() - rlg).abs().max())
    agree = float((lg.cpu().argmax(-1) == rlg.argmax(-1)).float().mean())
    free = float((tok == rtok).float().mean())
    # the same engine, fixed shape: per size, the 26 images of that size in one fixed-shape session (rows never interact)
    enc_solo = lg_solo = 0.0
    for k, size in enumerate(kinds):
        idx = list(range(k, 130, 5))
        x = torch.stack([dev[i] for i in idx])
        fe = m.encoder(x)
        enc_solo = max(enc_solo, float((enc[idx, :fe.shape[1]] - fe).abs().max()))
        assert bool((enc[idx, fe.shape[1]:] == 0).all())
        eng.decode_begin(fe)
        fl = torch.stack([eng.decode_step(t, prefix[t, idx].contiguous())[0] for t in range(steps)], 1)
        lg_solo = max(lg_solo, float((lg[idx] - fl).abs().max()))
    print(f"\n[ragged bf16 benchmark dims, 130 rows, two ranges] vs float64: encoder {enc_err:.4f} (bound {BENCH_BF16_ENC_BOUND:.4f}), teacher-forced "
          f"logits {err:.4f} (bound {BF16_BOUND['logits']:.4f}), top-1 agreement {agree:.4f} of {130 * steps}; free-running token agreement "
          f"{free:.4f}; vs the fixed-shape run: encoder {enc_solo:.2e}, step logits {lg_solo:.2e}")
    assert enc_err < BENCH_BF16_ENC_BOUND and err < BF16_BOUND["logits"] and agree >= 0.97
    assert enc_solo == 0.0 and lg_solo == 0.0


def _rc(eng, fn, *args):
    with torch.cuda.device(eng.device):
        rc = getattr(eng.lib, fn)(eng.handle, *args)
    return rc, eng.lib.txo_last_error().decode()


def test_refusals_and_no_state_leak():
    """test 8: every out-of-scope call answers TXO_E_INVALID with a message naming ragged batches; a fixed-shape generate directly after a
    ragged one is bit-identical to one before it"""
    d = TINY
    _, _, m = build(d, max_batch=4, max_tokens=40, seed=3)
    m.eos_token = None
    eng = m._engine
    x = torch.from_numpy(synth.synth_images(3, 3, 48, 80, seed=9)).cuda()
    before = m.generate(x, 12)
    images = [im.cuda() for im in _images([(32, 32), (48, 96), (16, 64)], 40)]
    box, sizes = ops.pack_ragged(images)
    out = torch.empty((4, 40, d.embed_dim), device="cuda")
    toks = torch.empty((4, 64), dtype=torch.int64, device="cuda")
    n = C.c_int32(0)
    I32 = C.POINTER(C.c_int32)

    def enc_call(sz, B=3, Hc=48, Wc=96):
        arr = (C.c_int32 * len(sz))(*sz)
        return _rc(eng, "txo_encode_ragged", box.data_ptr(), B, 3, Hc, Wc, C.cast(arr, I32), out.data_ptr(), C.byref(n), None)

    for sz, frag in (([32, 32, 40, 96, 16, 64], "multiples of 16"), ([32, 32, 64, 96, 16, 64], "container"),
                     ([32, 32, 48, 96, 16, 0], "multiples of 16"), ([32, 32, 48, 96, 128, 128], "container")):
        rc, msg = enc_call(sz)
        assert rc == _lib.TXO_E_INVALID and "ragged" in msg and frag in msg, (sz, rc, msg)
    big = torch.zeros((1, 3, 144, 144), device="cuda")
    arr = (C.c_int32 * 2)(144, 144)
    rc, msg = _rc(eng, "txo_encode_ragged", big.data_ptr(), 1, 3, 144, 144, C.cast(arr, I32), out.data_ptr(), C.byref(n), None)
    assert rc == _lib.TXO_E_INVALID and "canvas" in msg and "ragged" in msg, msg
    arr = (C.c_int32 * 2)(128, 128)                                         # 65 tokens > max_tokens = 40
    rc, msg = _rc(eng, "txo_encode_ragged", big.data_ptr(), 1, 3, 144, 144, C.cast(arr, I32), out.data_ptr(), C.byref(n), None)
    assert rc == _lib.TXO_E_INVALID and "max_tokens" in msg and "ragged" in msg, msg
    odd = torch.zeros((1, 3, 16, 18), device="cuda")
    arr = (C.c_int32 * 2)(16, 16)
    rc, msg = _rc(eng, "txo_encode_ragged", odd.data_ptr(), 1, 3, 16, 18, C.cast(arr, I32), out.data_ptr(), C.byref(n), None)
    assert rc == _lib.TXO_E_INVALID and "multiple of 4" in msg and "ragged" in msg, msg
    rc, msg = enc_call([16, 16] * 5, B=5)
    assert rc == _lib.TXO_E_INVALID and "max_batch" in msg and "ragged" in msg, msg
    arr = (C.c_int32 * 6)(*sizes.flatten().tolist())
    rc, msg = _rc(eng, "txo_generate_ragged", box.data_ptr(), 3, 3, 48, 96, C.cast(arr, I32), d.max_len + 1, -1, toks.data_ptr(), C.byref(n), None)
    assert rc == _lib.TXO_E_INVALID and "ragged" in msg and "max_len" in msg, msg
    # calls that have no ragged form, on a ragged session
    enc, ntok = m.encoder.forward_ragged(images)
    eng.decode_begin_ragged(enc, ntok)
    t3 = torch.full((3, 4), d.bos, dtype=torch.int64, device="cuda")
    f3 = torch.empty((3, 3), device="cuda")
    i3 = torch.empty((3, 3), dtype=torch.int64, device="cuda")
    mask = torch.ones((3, 4), dtype=torch.uint8, device="cuda")
    for fn, args in (("txo_decode_prefill", (t3.data_ptr(), 4, None, None)),
                     ("txo_decode_score", (t3.data_ptr(), 4, f3.data_ptr(), i3.data_ptr(), f3.data_ptr(), None)),
                     ("txo_decode_set_key_mask", (mask.data_ptr(), 4, None)),
                     ("txo_score", (x.data_ptr(), 3, 3, 48, 80, t3.data_ptr(), None, 4, f3.data_ptr(), i3.data_ptr(), f3.data_ptr(), None))):
        rc, msg = _rc(eng, fn, *args)
        assert rc == _lib.TXO_E_INVALID and "ragged" in msg, (fn, rc, msg)
    with pytest.raises(ValueError, match="ragged"):
        eng.decode_prefill(t3)
    # ... and the session still steps
    lg, _ = eng.decode_step(0, t3[:, 0].contiguous())
    assert bool(torch.isfinite(lg).all())
    r1 = m.generate_ragged(images, 12)
    assert eng.query(Q_LAST_RAGGED) == 1 and eng.query(Q_LAST_PERSISTENT) == 0
    # the ragged generate closed its session: the whole-pipeline scoring call behind it opens its own
    rc, msg = _rc(eng, "txo_score", x.data_ptr(), 3, 3, 48, 80, t3.data_ptr(), None, 4, f3.data_ptr(), i3.data_ptr(), f3.data_ptr(), None)
    assert rc == 0, msg
    after = m.generate(x, 12)
    assert eng.query(Q_LAST_RAGGED) == 0
    assert torch.equal(before, after), "a fixed-shape generate changed after a ragged one"
    assert torch.equal(r1, m.generate_ragged(images, 12))


@pytest.mark.parametrize("what,env", [("hybrid", None), ("latent", {"TXO_LATENT": "1"})])
def test_refused_front_end_and_cross_attention_form(what, env):
    """test 8: the hybrid front end and the forced latent cross-attention form refuse a ragged call"""
    if what == "hybrid":
        d = Dims(canvas=64, canvas_w=128, embed="hybrid", in_channels=1, embed_dim=64, enc_heads=1, enc_layers=1, dec_heads=1, dec_layers=1,
                 vocab=32, max_len=8, bos=30, eos=29, pad=31)
        images = [torch.zeros((1, 32, 64), device="cuda"), torch.zeros((1, 64, 32), device="cuda")]
    else:
        d = RAG_DIMS
        images = [torch.zeros((3, 32, 64), device="cuda"), torch.zeros((3, 64, 32), device="cuda")]
    _, _, m = build(d, seed=1, max_batch=2, env=env)
    with pytest.raises(ValueError, match="ragged batches.*(hybrid|latent)"):
        m.encoder.forward_ragged(images)
    with pytest.raises(ValueError, match="ragged batches.*(hybrid|latent)"):
        m.generate_ragged(images, 4)


def test_facades_equal_per_image_calls(tmp_path):
    """test 9: OCRModel.generate_ragged / VisionEncoder.forward_ragged / TeXOCRWrapper.batch over a list of PIL images longer than
    max_batch equal TeXOCRWrapper.__call__ per image (greedy, fp32)"""
    import json
    import os
    from PIL import Image
    from texocr_amd.config import default_config
    from texocr_amd.tokenizer import RegExTokenizer
    from texocr_amd.wrapper import TeXOCRWrapper, preprocess_image
    v = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tokenizer_vocab_1k.json")))
    RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"]).save(str(tmp_path / "vocab.txt"))
    cfg = default_config(img_size=[64, 256], max_length=32, in_channels=1,
                         encoder={"embed_dim": 64, "heads": 2, "num_layers": 1}, decoder={"embed_dim": 64, "heads": 2, "num_layers": 2})
    cfg["tokenizer_path"] = str(tmp_path / "vocab.txt")
    w = TeXOCRWrapper(cfg, max_batch=3)
    d = w.dims
    w.model.load_state_dict(synth.synth_state_dict(d, 5))
    rng = np.random.RandomState(0)
    pil = []
    for i, (wd, ht) in enumerate([(200, 40), (30, 30), (250, 64), (100, 17), (64, 64), (16, 48), (130, 33)]):
        a = np.full((ht, wd, 3), 255, dtype=np.uint8)
        a[rng.randint(0, ht, 40), rng.randint(0, wd, 40)] = rng.randint(0, 120, (40, 1))
        pil.append(Image.fromarray(a))
    one = [w(im, max_len=20, decode="greedy") for im in pil]
    got = w.batch(pil, max_len=20, decode="greedy")
    assert len(got) == len(pil) == 7 > w.model._engine.max_batch
    for b, (a, g) in enumerate(zip(one, got)):
        assert a[0] == g[0] and a[1] == g[1], (b, a, g)
    xs = [preprocess_image(im).cuda() for im in pil[:3]]
    enc, ntok = w.model.encoder.forward_ragged(xs)
    for b, x in enumerate(xs):
        solo = w.model.encoder(x[None])[0]
        assert float((enc[b, :int(ntok[b])] - solo).abs().max()) < 1e-4 and bool((enc[b, int(ntok[b]):] == 0).all())
    w.model.eos_token = None
    t = w.model.generate_ragged(xs, 10)
    for b, x in enumerate(xs):
        assert torch.equal(t[b], w.model.generate(x[None], 10)[0]), b
