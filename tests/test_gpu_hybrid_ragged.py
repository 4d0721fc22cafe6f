"""Ragged batches on the hybrid ResNetV2 front end (txo_set_ragged_hybrid; csrc/conv.h: the RAGGED forms), on the GPU.

A small ViT (width 64, one encoder and one decoder layer) behind the real backbone on the reference canvas (160, 1008); weights synth seed 9,
images synth seed 31 + slot, as tests/test_gpu_hybrid.py.  The mixed list takes its sizes from that file's SIZES, each a known edge:
    slot 0  64x320    sets the container height
    slot 1  16x16     a GroupNorm over one pixel at the last stage; n_b = 2
    slot 2  32x256    HW = 128
    slot 3  48x176    HW = 132; odd stage width 11
    slot 4  16x1008   sets the container width; stage width 63
    slot 5  a copy of slot 1, slot 6 a copy of slot 3 (copies in different slots)
A second case holds one 160x1008 image beside a 16x16 one: the small image's extent is a sliver of every tile.

Reference: the float64 run of oracle/cpu_ref.py (tests/ref64.py) on every image ALONE.  Bounds are the ones tests/test_gpu_hybrid.py asserts
for the same kernels; none comes from the engine:
- fp32 engine: max |enc - enc64| < 5e-4;
- bf16 default and TXO_BACKBONE_EXACT=1: per_image_rel < 0.02, worst image;
- TXO_BACKBONE_BF16=1: as that file holds it -- against the float64 run with every stored backbone tensor rounded to bf16, < 0.1, on the
  sizes that file holds it on (32x256, 48x176, 64x320: slots 0, 2, 3, 6);
- a ragged row against the same engine's solo encoder(img[None]): torch.equal in the fp32 engine and in the bf16 engines with
  TXO_BACKBONE_EXACT=1 / TXO_BACKBONE_BF16=1 (solo statistics from gn_partial_kernel, whose ragged form repeats the solo partials bit for
  bit; GEMM rows do not depend on M); in the default bf16 engine the solo run takes the fused statistics of gemm_split.h, so
  per_image_rel(ragged, solo) < 0.02, the bound that file gives copy against copy;
- copies of one image in different slots: bit-identical in every engine kind (all ragged statistics are unfused and per image).
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import ref64
from gpu_harness import assert_tokens_exact_up_to_margin, build, oracle, per_image_rel
from texocr_amd import _lib, ops, synth
from texocr_amd.config import Dims

pytestmark = pytest.mark.gpu

WEIGHT_SEED, IMAGE_SEED = 9, 31
DIMS = Dims(canvas=160, canvas_w=1008, embed="hybrid", in_channels=1, embed_dim=64, enc_heads=1, enc_layers=1, dec_heads=1, dec_layers=1,
            vocab=64, max_len=16, bos=62, eos=61, pad=63)
MIXED = [(64, 320), (16, 16), (32, 256), (48, 176), (16, 1008)]
COPIES = {5: 1, 6: 3}
SLIVER = [(160, 1008), (16, 16)]
BF16_BACKBONE_SLOTS = (0, 2, 3, 6)                             # tests/test_gpu_hybrid.py: BF16_BACKBONE_SIZES
FP32_BOUND, BF16_BOUND, BF16_BACKBONE_BOUND = 5e-4, 0.02, 0.1
FP32_LOGP = 2e-4                                               # tests/test_gpu_logp.py
KINDS = {"fp32": ("fp32", {}), "bf16": ("bf16", {}), "exact": ("bf16", {"TXO_BACKBONE_EXACT": "1"}),
         "bf16bk": ("bf16", {"TXO_BACKBONE_BF16": "1"})}


@functools.lru_cache(maxsize=None)
def weights():
    sd = synth.synth_state_dict(DIMS, WEIGHT_SEED)
    return sd, ref64.sd64(sd)


def _image(i, h, w):
    return torch.from_numpy(synth.synth_images(1, 1, h, w, seed=IMAGE_SEED + i))[0]


@functools.lru_cache(maxsize=None)
def mixed():
    """(images (1, H_b, W_b) on the host, float64 encoder rows of each image alone)"""
    images = [_image(i, h, w) for i, (h, w) in enumerate(MIXED)]
    images += [images[COPIES[5]].clone(), images[COPIES[6]].clone()]
    enc64 = [ref64.encode(weights()[1], im[None], grid_w=DIMS.grid)[0] for im in images[:5]]
    enc64 += [enc64[COPIES[5]], enc64[COPIES[6]]]
    return images, enc64


@functools.lru_cache(maxsize=None)
def sliver():
    images = [_image(10 + i, h, w) for i, (h, w) in enumerate(SLIVER)]
    return images, [ref64.encode(weights()[1], im[None], grid_w=DIMS.grid)[0] for im in images]


def model(kind, max_batch=7, env=None, on=True):
    dtype, create = KINDS[kind]
    m = build(DIMS, dtype=dtype, max_batch=max_batch, sd=weights()[0], env=dict(create, **(env or {})))[2]
    m.eos_token = None
    if on:
        m.ragged_hybrid = True
    return m


def cuda(images):
    return [im.cuda() for im in images]


def rows(enc, ntok, b):
    return enc[b, :int(ntok[b])].cpu()


def rel1(a, ref, scale=None):
    return float(per_image_rel(a[None], ref[None], scale=None if scale is None else scale[None])[0])


def check_against_float64(kind, enc, ntok, images, enc64, slots_bf16bk=()):
    """test 1: per image against float64, padding rows exactly zero, n_tokens"""
    worst = 0.0
    assert enc.shape == (len(images), max(e.shape[0] for e in enc64), DIMS.embed_dim)
    emu_q = (lambda x: oracle().bf16_round(x).to(x.dtype)) if kind == "bf16bk" else None
    for b, im in enumerate(images):
        n = 1 + (im.shape[1] // 16) * (im.shape[2] // 16)
        assert int(ntok[b]) == n == enc64[b].shape[0], b
        assert bool((enc[b, n:] == 0).all()), f"padding rows of slot {b} are not zero"
        got = rows(enc, ntok, b)
        assert bool(torch.isfinite(got).all()), b
        if kind == "fp32":
            err = float((got.double() - enc64[b]).abs().max())
            assert err < FP32_BOUND, f"fp32, slot {b} {tuple(im.shape[1:])}: max |enc - enc64| {err:.3e} >= {FP32_BOUND:g}"
        elif kind == "bf16bk":
            if b not in slots_bf16bk:
                continue
            emu = ref64.encode(weights()[1], im[None], grid_w=DIMS.grid, backbone_q=emu_q)[0]
            err = rel1(got, emu, scale=enc64[b])
            assert err < BF16_BACKBONE_BOUND, f"bf16 backbone, slot {b} {tuple(im.shape[1:])}: vs emulation {err:.4f} >= {BF16_BACKBONE_BOUND}"
        else:
            err = rel1(got, enc64[b])
            assert err < BF16_BOUND, f"{kind}, slot {b} {tuple(im.shape[1:])}: per_image_rel {err:.5f} >= {BF16_BOUND}"
        worst = max(worst, err)
    return worst


def check_against_solo(kind, m, enc, ntok, images):
    """test 2: every ragged row against the same engine's solo run"""
    worst = 0.0
    for b, im in enumerate(images):
        solo = m.encoder(im[None].cuda())[0].cpu()
        got = rows(enc, ntok, b)
        if kind == "bf16":
            r = rel1(got, solo)
            worst = max(worst, r)
            assert r < BF16_BOUND, f"bf16 default, slot {b} {tuple(im.shape[1:])}: ragged vs solo {r:.5f} >= {BF16_BOUND}"
        else:
            assert torch.equal(got, solo), f"{kind}, slot {b} {tuple(im.shape[1:])}: the ragged rows differ from the solo run by " \
                                           f"{float((got - solo).abs().max()):.3e}"
    return worst


@pytest.mark.parametrize("kind", list(KINDS))
def test_mixed_list_per_image_against_float64_and_solo(kind):
    images, enc64 = mixed()
    m = model(kind)
    enc, ntok = m.encoder.forward_ragged(cuda(images))
    w64 = check_against_float64(kind, enc, ntok, images, enc64, BF16_BACKBONE_SLOTS)
    for slot, first in COPIES.items():
        assert torch.equal(enc[slot], enc[first]), f"{kind}: slots {slot} and {first} hold the same image and differ by " \
                                                   f"{float((enc[slot] - enc[first]).abs().max()):.3e}"
    wsolo = check_against_solo(kind, m, enc, ntok, images)
    print(f"\nragged hybrid, mixed list, {kind}: worst image vs float64 {w64:.3e}; ragged vs solo "
          f"{'%.5f (bound %g)' % (wsolo, BF16_BOUND) if kind == 'bf16' else 'bit-identical'}")


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_full_canvas_beside_the_smallest_image(kind):
    images, enc64 = sliver()
    m = model(kind, max_batch=2)
    enc, ntok = m.encoder.forward_ragged(cuda(images))
    w64 = check_against_float64(kind, enc, ntok, images, enc64)
    wsolo = check_against_solo(kind, m, enc, ntok, images)
    print(f"\nragged hybrid, 160x1008 beside 16x16, {kind}: worst image vs float64 {w64:.3e}; ragged vs solo {wsolo:.5f}")


def _fill_outside(box, sizes, value):
    out = torch.full_like(box, value)
    for b, (h, w) in enumerate(sizes.tolist()):
        out[b, :, :h, :w] = box[b, :, :h, :w]
    return out


def test_nothing_outside_the_corners_is_read():
    """test 3: NaN, then 1e30, everywhere outside the corners: encoder rows and generate_ragged tokens are bit-identical to the zero-filled
    run; a NaN pixel inside image 2 leaves every other slot bit-identical"""
    images, _ = mixed()
    m = model("fp32")
    eng = m._engine
    box, sizes = ops.pack_ragged(cuda(images))
    assert box.shape == (7, 1, 64, 1008)

    def run(container):
        enc = torch.ops.texocr.encode_ragged(container, sizes, eng.id)
        toks, n = torch.ops.texocr.generate_ragged(container, sizes, eng.id, 8, -1)
        return enc, toks[:, :int(n.item())]

    base = run(box)
    assert bool(torch.isfinite(base[0]).all())
    for value in (float("nan"), 1e30):
        got = run(_fill_outside(box, sizes, value))
        for a, b, name in zip(base, got, ("encoder", "tokens")):
            assert torch.equal(a, b), f"{name} changed with {value} outside the corners"
    bad = box.clone()
    bad[2, 0, 3, 5] = float("nan")                             # inside image 2 (32x256)
    got = run(bad)
    others = [b for b in range(7) if b != 2]
    for a, b, name in zip(base, got, ("encoder", "tokens")):
        assert torch.equal(a[others], b[others]), f"{name} of another slot changed with a NaN inside image 2"
    assert torch.equal(run(box)[0], base[0])                   # (and what that run left in the workspaces reaches nothing)


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_all_sizes_equal_matches_the_fixed_shape_call(kind):
    """test 4: five 48x176 images: the ragged call equals encoder(x) -- exactly in fp32, within the ragged-vs-solo bound in default bf16"""
    x = torch.cat([_image(20 + i, 48, 176)[None] for i in range(5)]).cuda()
    m = model(kind)
    enc, ntok = m.encoder.forward_ragged(list(x))
    fixed = m.encoder(x)
    assert enc.shape == fixed.shape and ntok.tolist() == [34] * 5
    if kind == "fp32":
        assert torch.equal(enc, fixed), float((enc - fixed).abs().max())
    else:
        r = per_image_rel(enc, fixed)
        print(f"\nragged hybrid, five 48x176, bf16 default: ragged vs fixed shape, worst image {float(r.max()):.5f} (bound {BF16_BOUND})")
        assert float(r.max()) < BF16_BOUND


def test_stale_state_between_fixed_and_ragged_encodes_bf16():
    """test 5: a ragged encode right after a fixed-shape bf16 encode of a larger batch does not read the gn_tiles it left; a fixed-shape
    bf16 encode right after a ragged one equals the same encode on a fresh engine"""
    images, enc64 = mixed()
    x = torch.cat([_image(20 + i, 48, 176)[None] for i in range(7)]).cuda()
    fresh = model("bf16")
    enc_fresh, ntok = fresh.encoder.forward_ragged(cuda(images))
    m = model("bf16")
    fixed_first = m.encoder(x)                                 # (fused statistics: gn_tiles written)
    enc_after, _ = m.encoder.forward_ragged(cuda(images))
    assert torch.equal(enc_after, enc_fresh), float((enc_after - enc_fresh).abs().max())
    fixed_after = m.encoder(x)
    assert torch.equal(fixed_after, fixed_first), float((fixed_after - fixed_first).abs().max())
    check_against_float64("bf16", enc_after, ntok, images, enc64)


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_image_chunks_of_3_over_the_seven_slots(kind):
    """test 5: TXO_ENC_CHUNK=3 (chunks of 3, 3, 1 images) is bit-identical to the unchunked ragged encode"""
    images, _ = mixed()
    whole, _ = model(kind).encoder.forward_ragged(cuda(images))
    chunked, _ = model(kind, env={"TXO_ENC_CHUNK": "3"}).encoder.forward_ragged(cuda(images))
    assert torch.equal(whole, chunked), float((whole - chunked).abs().max())


def test_generate_score_align_rows_equal_the_per_image_calls_fp32():
    """test 6: generate_ragged(stop='row', return_logp=True), score_ragged and align_ragged against the calls on every image alone"""
    images, enc64 = mixed()
    d = DIMS
    m = model("fp32")
    m.eos_token = d.eos
    dev = cuda(images)
    steps = 10
    toks, logp = m.generate_ragged(dev, steps, stop="row", return_logp=True)
    toks, logp = toks.cpu(), logp.cpu()
    trg = torch.cat([torch.full((7, 1), d.bos, dtype=torch.int64), torch.randint(0, 60, (7, 9), generator=torch.Generator().manual_seed(4))], 1).cuda()
    score = m.score_ragged(dev, trg)
    align = m.align_ragged(dev, trg)
    for b, im in enumerate(dev):
        ref_t, ref_l = ref64.generate(weights()[1], enc64[b][None], d.bos, d.eos, steps, stop="row", pad=d.pad)
        n = min(ref_t.shape[1], toks.shape[1])
        assert_tokens_exact_up_to_margin(toks[b:b + 1, :n].numpy(), ref_t[:, :n].numpy(), ref_l[:, :n])
        t1, p1 = m.generate(im[None], steps, stop="row", return_logp=True)
        n = min(t1.shape[1], toks.shape[1])
        assert torch.equal(toks[b, :n], t1[0, :n].cpu()), (b, toks[b].tolist(), t1[0].tolist())
        assert float((logp[b, :n] - p1[0, :n].cpu()).abs().max()) < FP32_LOGP, b
        s1 = m.score(im[None], trg[b:b + 1])
        assert torch.equal(score.top1[b], s1.top1[0]) and float((score.logp[b] - s1.logp[0]).abs().max()) < FP32_LOGP, b
        a1 = m.align(im[None], trg[b:b + 1])
        h, w = im.shape[1] // 16, im.shape[2] // 16
        assert align[b].maps.shape == (1, trg.shape[1] - 1, h, w) == a1.maps.shape, (b, align[b].maps.shape)
        assert float((align[b].maps - a1.maps).abs().max()) < 1e-5, b
    for slot, first in COPIES.items():
        assert torch.equal(toks[slot], toks[first]) and torch.equal(logp[slot], logp[first])


def test_wrapper_batch_equals_per_image_calls(tmp_path):
    """test 6: TeXOCRWrapper(config, ragged_hybrid=True).batch(pil_images) equals __call__ per image (greedy, fp32)"""
    from PIL import Image
    from texocr_amd.config import default_config
    from texocr_amd.tokenizer import RegExTokenizer
    from texocr_amd.wrapper import TeXOCRWrapper
    v = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tokenizer_vocab_1k.json")))
    RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"]).save(str(tmp_path / "vocab.txt"))
    cfg = default_config(img_size=[160, 1008], max_length=16, in_channels=1, embed="hybrid",
                         encoder={"embed_dim": 64, "heads": 1, "num_layers": 1}, decoder={"embed_dim": 64, "heads": 1, "num_layers": 1})
    cfg["tokenizer_path"] = str(tmp_path / "vocab.txt")
    w = TeXOCRWrapper(cfg, max_batch=3, ragged_hybrid=True)
    assert w.dims.embed == "hybrid" and w.model.ragged_hybrid
    w.model.load_state_dict(synth.synth_state_dict(w.dims, 5))
    rng = np.random.RandomState(0)
    pil = []
    for wd, ht in [(200, 40), (30, 30), (250, 64), (100, 17)]:
        a = np.full((ht, wd, 3), 255, dtype=np.uint8)
        a[rng.randint(0, ht, 40), rng.randint(0, wd, 40)] = rng.randint(0, 120, (40, 1))
        pil.append(Image.fromarray(a))
    one = [w(im, max_len=8, decode="greedy") for im in pil]
    got = w.batch(pil, max_len=8, decode="greedy")
    assert len(got) == len(pil) == 4 > w.model._engine.max_batch
    for b, (a, g) in enumerate(zip(one, got)):
        assert a[0] == g[0] and a[1] == g[1], (b, a, g)


def test_the_switch():
    """test 7: off, the refusal and its message stay; values other than 0 / 1 are refused at the C ABI; TXO_LATENT=1 refuses with it on"""
    images = cuda(mixed()[0][:3])
    m = model("fp32", max_batch=3, on=False)
    assert m.ragged_hybrid is False
    for call in (lambda: m.encoder.forward_ragged(images), lambda: m.generate_ragged(images, 4)):
        with pytest.raises(ValueError, match="ragged batches.*hybrid"):
            call()
    eng = m._engine
    for bad in (2, -1):
        assert eng.lib.txo_set_ragged_hybrid(eng.handle, bad) == _lib.TXO_E_INVALID
        assert "txo_set_ragged_hybrid" in eng.lib.txo_last_error().decode()
    with pytest.raises(ValueError):
        m.ragged_hybrid = 2
    m.ragged_hybrid = True
    enc, ntok = m.encoder.forward_ragged(images)
    assert ntok.tolist() == [81, 2, 33] and m.ragged_hybrid is True
    m.load_state_dict(weights()[0])                            # (a reload makes a new engine handle: the switch follows the model)
    assert torch.equal(m.encoder.forward_ragged(images)[0], enc)
    m.ragged_hybrid = False
    with pytest.raises(ValueError, match="ragged batches.*hybrid"):
        m.encoder.forward_ragged(images)
    lat = build(DIMS, dtype="fp32", max_batch=3, sd=weights()[0], latent=1)[2]
    lat.ragged_hybrid = True
    with pytest.raises(ValueError, match="ragged batches.*latent"):
        lat.encoder.forward_ragged(images)
