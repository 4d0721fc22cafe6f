"""The hybrid ResNetV2 front end (csrc/conv.h, csrc/gemm_split.h) judged PER IMAGE, over batch sizes and image shapes.

The backbone is the one place in the engine where rows of different images meet inside a kernel tile: a 128-row GEMM tile of a
convolution covers pixels of up to two images, and in the default bf16 engine the tile's epilogue writes the GroupNorm partial sums of
both (gemm_split.h: GnPart, `split`, `which`; gn_finish_tiles_kernel).  Which rows of which tile belong to which image depends on
b * HW mod 128: on the slot of the image in the batch and on its size together.  From 128 pixels per image on a GroupNorm takes this
fused form; below it gn_partial_kernel / gn_finish_kernel (conv.h) run.  A batch mean hides wrong statistics of one image of 64 behind
a weight of 1/64, so every relative figure here is the MAXIMUM over the images of a batch of
    per_image_rel = mean |enc - enc64| over the image's tokens and columns / mean |enc64| of that image.

Reference throughout: the float64 run of oracle/cpu_ref.py (tests/ref64.py), weights synth seed 9, images synth seed 31.

Batches of S slots are filled from n distinct images by the pattern slot i -> image (5 i + i // 7) % n, so that
- every slot is held against the float64 rows of its image, and
- the copies of one image are held against each other: bit-identical in the fp32 engine and in the bf16 engine with
  TXO_BACKBONE_EXACT=1 (statistics from gn_partial_kernel, whose chunks are per image; GEMM rows are independent); in the default bf16
  engine the fused sums are cut at `split`, which differs from slot to slot, so there copy against copy is held to the per-image bound.

Bounds (none of them comes from the engine):
- fp32 engine: max |enc - enc64| < min(5e-4, max(5e-4, 4 * e32(size))) = 5e-4, e32 = the reference's own fp32 error against its float64 run on the same
  images, measured on a CPU (oracle/cpu_ref.py in fp32 against float64, max abs over the distinct images of the size):
      size       e32        per image, relative
      16x16      9.1e-05    1.1e-05 - 2.0e-05
      32x256     1.0e-04    1.1e-05 - 1.3e-05
      48x176     9.6e-05    1.3e-05 - 1.4e-05
      16x1008    7.6e-05    9.8e-06 - 1.0e-05
      64x320     1.2e-04    1.3e-05 - 1.4e-05
      160x1008   1.4e-04    1.5e-05
  4 * e32 stays below 5e-4 at every size but the full canvas (5.5e-4 over its four images); there the bound is kept at the 5e-4 that the
  suite asserts on the full canvas already, so it is 5e-4 (4-5x the reference's own fp32 error) at every size.
- default bf16 engine and TXO_BACKBONE_EXACT=1 against float64: per-image relative error < 0.02 (the bound the suite held the batch
  mean to, moved to the worst image).  Rounding every tensor the backbone stores to 17 significant bits moves the float64 result by
  5e-4 per image; the rest of the measured error is the bf16 ViT behind the backbone.
- default bf16 against TXO_BACKBONE_EXACT=1, same slots: per image < 0.01.  The two share the bf16 ViT kernel for kernel and differ by the
  split product's error and the order of the GroupNorm sums; the exact variant takes its statistics from the unfused kernels that the
  fp32 engine pins to float64.  This is the sharpest of the three for a tile attributed to the wrong image.
- TXO_BACKBONE_BF16=1 (32x256, 48x176, 64x320): against the float64 run with every stored backbone tensor rounded to bf16
  (cpu_ref.bf16_round), as tests/test_gpu_parity.py::test_hybrid_oracle_wider_image_and_bf16 judges it, per image.

Measured on MI355X (worst image over all slot counts of the size; `copies` = the largest copy-to-copy difference in the default bf16
engine, relative like the rest):
      size       fp32 max abs   bf16 default   bf16 exact   default vs exact   copies    bf16 backbone vs emulation
      16x16      1.60e-04       0.0076         0.0077       0.0068             0         -
      32x256     1.15e-04       0.0054         0.0053       0.0044             0         0.070
      48x176     1.16e-04       0.0055         0.0053       0.0047             0.0044    0.086
      16x1008    9.03e-05       0.0056         0.0055       0.0044             0.0042    -
      64x320     1.35e-04       0.0053         0.0053       0.0043             0         0.084
      160x1008   1.52e-04       0.0052         0.0052       0.0040             0.0037    -
  bound          5e-4           0.02           0.02         0.01               0.02      0.1
(copies are bit-identical in the default bf16 engine where every image starts on a 64-row seam at every fused resolution -- the epilogue
sums per 64-row half of a tile, so an image that starts on a half-tile seam, as at 64x320 with HW = 320 at stage 1, gets the same
partial sums in the same order as one that starts on a tile seam; in the TXO_BACKBONE_BF16=1 engine they are bit-identical at every
size, asserted: its statistics come from gn_partial_kernel.  Split against
exact is 0.7 % at 16x16, where no GroupNorm is fused: it is the split product's 2^-17 seen through the bf16 ViT, whose roundings turn
any last-bit difference of its input into 0.4 %, as copy against copy shows.)

One-line mutations of the engine, each run once against this module and against the five older hybrid tests of test_gpu_parity.py:
  1 gemm_split.h: all rows of a tile counted for its first image   test_bf16_engines_every_slot_per_image[48x176, 16x1008, 64x320, 160x1008],
                                                                   test_image_chunks_of_7_at_33_slots; the older batch means fail too (8-20 %)
  2 `in1` without `r < mlim`, rows beyond M staged as ones         passes everything, and cannot matter: with HW >= 128 the last row tile lies
                                                                   wholly in the last image, which reads its which = 0 slot only
  3 gn_finish_tiles_kernel: t1 without the - 1                     test_tile_sums_left_by_an_earlier_encode_are_not_read only; the older tests pass
  4 gn_finish_tiles_kernel: `which` always 0                       as 1; the older batch means fail too (12-13 %)
  5 group_norm: nchunk rounded down                                20 of 21 here and 4 of 5 older ones (an empty grid is a launch error)
  6 max pool padded with 0                                         passes everything, and cannot matter: the pool's input is behind a ReLU and
                                                                   every window holds a valid pixel
  7 gn_fusable: HW > 128                                           passes everything: HW = 128 then takes the unfused form, which is as correct
"""
import functools

import pytest
import torch

import ref64
from gpu_harness import assert_tokens_exact_up_to_margin, build, oracle, per_image_rel
from texocr_amd import synth
from texocr_amd.config import Dims, reference_config

pytestmark = pytest.mark.gpu

WEIGHT_SEED, IMAGE_SEED = 9, 31
GB_BM = 128                                                    # rows of a GEMM tile (csrc/gemm_big.h)

# size: (H, W, distinct images, slot counts)
SMALL_SLOTS = (1, 2, 3, 5, 17, 33, 64)
SIZES = {
    "16x16": (16, 16, 6, SMALL_SLOTS),                         # smallest image; a GroupNorm over one pixel; N = 2
    "32x256": (32, 256, 6, SMALL_SLOTS),                       # HW = 128 exactly: the image boundary on the tile seam
    "48x176": (48, 176, 6, SMALL_SLOTS),                       # HW = 132: every tile but the first straddles, 32 values of `split`
    "16x1008": (16, 1008, 6, SMALL_SLOTS),                     # one token row at full canvas width; odd stage width 63
    "64x320": (64, 320, 4, (3, 17, 64)),                       # the size the older tests have, now at 64 slots
    "160x1008": (160, 1008, 4, (1, 2, 5)),                     # full canvas
}
BF16_BACKBONE_SIZES = ("32x256", "48x176", "64x320")

# the reference's own fp32 error against its float64 run, max abs (table in the header)
E32 = {"16x16": 9.12e-5, "32x256": 1.00e-4, "48x176": 9.55e-5, "16x1008": 7.56e-5, "64x320": 1.15e-4, "160x1008": 1.37e-4}
BF16_BOUND, SPLIT_VS_EXACT_BOUND = 0.02, 0.01


def fp32_bound(size):
    return min(5e-4, max(5e-4, 4 * E32[size]))                  # never above what the older full-canvas test asserts


# engine kind: (storage type, what the engine reads when it is created)
KINDS = {"fp32": ("fp32", {}), "bf16": ("bf16", {}), "exact": ("bf16", {"TXO_BACKBONE_EXACT": "1"}),
         "bf16bk": ("bf16", {"TXO_BACKBONE_BF16": "1"})}

STAGES = ("stem", "stage 0", "stage 1", "stage 2")
# channel counts that meet a GroupNorm at each resolution (the first block of stages 1 and 2 normalises its first convolution at the
# resolution it comes from)
STAGE_CHANNELS = ((64,), (64, 256, 128), (128, 512, 256), (256, 1024))
# which resolutions take the fused statistics in the default bf16 engine: what the cases above are chosen for
EXPECT_FUSED = {"16x16": (False, False, False, False), "32x256": (True, True, True, False), "48x176": (True, True, True, False),
                "16x1008": (True, True, True, False), "64x320": (True, True, True, False), "160x1008": (True, True, True, True)}
EXPECT_HW = {"16x16": (64, 16, 4, 1), "32x256": (2048, 512, 128, 32), "48x176": (2112, 528, 132, 33), "16x1008": (4032, 1008, 252, 63),
             "64x320": (5120, 1280, 320, 80), "160x1008": (40320, 10080, 2520, 630)}


def gn_fusable(hw, c):
    """csrc/gemm_split.h: gn_fusable, restated (the C ABI does not say which GroupNorm form ran)"""
    cpg = c // 32
    return hw >= GB_BM and c % 32 == 0 and 1 <= cpg <= 32 and cpg & (cpg - 1) == 0


def stage_hw(H, W):
    """pixels per image at the stem / stage 0 / 1 / 2"""
    return tuple((H >> k) * (W >> k) for k in (1, 2, 3, 4))


def stage_fused(H, W):
    return tuple(all(gn_fusable(hw, c) for c in chans) for hw, chans in zip(stage_hw(H, W), STAGE_CHANNELS))


def slot_images(S, n):
    """which of n distinct images sits in each of S slots (repeats at slots of different b * HW mod 128)"""
    return [(5 * i + i // 7) % n for i in range(S)]


def where(size, slot):
    H, W = SIZES[size][:2]
    hw = stage_hw(H, W)
    forms = ", ".join(f"{s} {'fused' if f else 'unfused'}" for s, f in zip(STAGES, stage_fused(H, W)))
    return f"slot {slot} of {size}: b * HW mod 128 = {[slot * p % GB_BM for p in hw]} (HW {list(hw)}); GroupNorm: {forms}"


def assert_each_image_below(rel, bound, size, what):
    worst = int(rel.argmax())
    assert float(rel[worst]) < bound, f"{what}: {float(rel[worst]):.3e} >= {bound:g} at {where(size, worst)}"
    return float(rel[worst])


def copies_of(ids):
    """[(first slot, later slot)] for every slot that repeats an earlier slot's image"""
    first = {}
    return [(first[k], i) for i, k in enumerate(ids) if first.setdefault(k, i) != i]


def assert_copies_bit_identical(enc, ids, size, what):
    for a, b in copies_of(ids):
        assert torch.equal(enc[a], enc[b]), f"{what}: slots {a} and {b} hold the same image and differ by " \
                                            f"{float((enc[a] - enc[b]).abs().max()):.3e}; {where(size, b)}"


def copy_to_copy_rel(enc, ids, enc64):
    """(B,) per_image_rel of every slot against the first slot that holds its image (0 for the first ones)"""
    ref = enc.clone().double()
    for a, b in copies_of(ids):
        ref[b] = enc[a].double()
    return per_image_rel(enc, ref, scale=enc64)


@functools.lru_cache(maxsize=None)
def dims():
    d = Dims.from_config(reference_config())
    assert d.embed == "hybrid" and d.canvas_hw == (160, 1008) and d.in_channels == 1
    return d


@functools.lru_cache(maxsize=None)
def weights():
    sd = synth.synth_state_dict(dims(), WEIGHT_SEED)
    return sd, ref64.sd64(sd)


@functools.lru_cache(maxsize=2)
def reference(size):
    """the distinct images of a size and their float64 encoder rows"""
    H, W, n, _ = SIZES[size]
    img = torch.from_numpy(synth.synth_images(n, 1, H, W, seed=IMAGE_SEED))
    enc64 = ref64.encode(weights()[1], img, grid_w=dims().grid)
    assert enc64.dtype == torch.float64 and enc64.shape == (n, 1 + (H // 16) * (W // 16), dims().embed_dim)
    return img, enc64


def engine(kind, size, max_batch=64, max_tokens=None, env=None):
    """one engine per (kind, size) serves all slot counts: max_batch 64, max_tokens to fit the size"""
    H, W = SIZES[size][:2]
    dtype, create = KINDS[kind]
    fit = 1 + (H // 16) * (W // 16)
    return build(dims(), dtype=dtype, max_batch=max_batch, max_tokens=fit if max_tokens is None else max_tokens, sd=weights()[0],
                 env=dict(create, **(env or {})))[2]


def batch(size, S):
    img, enc64 = reference(size)
    ids = slot_images(S, SIZES[size][2])
    return ids, img[ids].cuda(), enc64[ids]


def encode(m, img, size):
    H, W = SIZES[size][:2]
    enc = m.encoder(img).cpu()
    assert enc.shape == (img.shape[0], 1 + (H // 16) * (W // 16), dims().embed_dim) and bool(torch.isfinite(enc).all())
    return enc


# ------------------------------------------------------------------------------------------------
def test_the_sizes_reach_the_groupnorm_forms_the_table_claims():
    """the cases are chosen by pixels per image; this keeps the table, gn_fusable as restated here and the cases from drifting apart"""
    for size, (H, W, n, slots) in SIZES.items():
        assert stage_hw(H, W) == EXPECT_HW[size], size
        for hw, chans in zip(stage_hw(H, W), STAGE_CHANNELS):
            assert len({gn_fusable(hw, c) for c in chans}) == 1, (size, hw)        # a resolution takes one form for all its norms
        assert stage_fused(H, W) == EXPECT_FUSED[size], size
        assert 4 <= n <= 6 and len(set(slot_images(max(slots), n))) == n
    assert not gn_fusable(127, 64) and gn_fusable(128, 64) and not gn_fusable(128, 96) and gn_fusable(128, 1024)
    # 32x256: the boundary of every image on a tile seam at the three fused resolutions; 48x176: `split` takes 32 values over 32 slots
    assert all(hw % GB_BM == 0 for hw in EXPECT_HW["32x256"][:3])
    assert len({b * 132 % GB_BM for b in range(32)}) == 32
    # 5 i + i // 7 puts the copies of an image at slots of different parity and tile phase
    ids = slot_images(64, 6)
    assert all(len({i % 2 for i, k in enumerate(ids) if k == img}) == 2 for img in range(6))


@pytest.mark.parametrize("size", list(SIZES))
def test_fp32_engine_every_slot_against_float64(size):
    H, W, n, slots = SIZES[size]
    bound = fp32_bound(size)
    m = engine("fp32", size)
    worst = 0.0
    for S in slots:
        ids, img, enc64 = batch(size, S)
        enc = encode(m, img, size)
        err = (enc.double() - enc64).abs().amax(dim=(1, 2))
        worst = max(worst, assert_each_image_below(err, bound, size, f"fp32 engine, {S} slots, max |enc - enc64|"))
        assert_copies_bit_identical(enc, ids, size, f"fp32 engine, {S} slots")
    print(f"\nhybrid {size} fp32: max |enc - enc64| over slots {slots}: {worst:.2e} (bound {bound:g})")


@pytest.mark.parametrize("size", list(SIZES))
def test_bf16_engines_every_slot_per_image(size):
    """the default bf16 engine (split GEMM + fused statistics) and TXO_BACKBONE_EXACT=1 (exact-f32 GEMM + unfused statistics)"""
    H, W, n, slots = SIZES[size]
    m_split, m_exact = engine("bf16", size), engine("exact", size)
    w_split = w_exact = w_ab = w_copy = 0.0
    for S in slots:
        ids, img, enc64 = batch(size, S)
        a, b = encode(m_split, img, size), encode(m_exact, img, size)
        assert not torch.equal(a, b)                                        # (two different kernels did run)
        w_exact = max(w_exact, assert_each_image_below(per_image_rel(b, enc64), BF16_BOUND, size, f"bf16 exact backbone, {S} slots, vs float64"))
        assert_copies_bit_identical(b, ids, size, f"bf16 exact backbone, {S} slots")
        w_split = max(w_split, assert_each_image_below(per_image_rel(a, enc64), BF16_BOUND, size, f"bf16 default, {S} slots, vs float64"))
        rel_ab = per_image_rel(a, b, scale=enc64)
        w_ab = max(w_ab, assert_each_image_below(rel_ab, SPLIT_VS_EXACT_BOUND, size, f"bf16 default vs exact backbone, {S} slots"))
        w_copy = max(w_copy, assert_each_image_below(copy_to_copy_rel(a, ids, enc64), BF16_BOUND, size, f"bf16 default, {S} slots, copy vs copy"))
    print(f"\nhybrid {size} bf16, worst image over slots {slots}: default vs float64 {w_split:.5f}, exact vs float64 {w_exact:.5f} "
          f"(bound {BF16_BOUND}); default vs exact {w_ab:.5f} (bound {SPLIT_VS_EXACT_BOUND}); default copy vs copy {w_copy:.5f}")


@pytest.mark.parametrize("size", BF16_BACKBONE_SIZES)
def test_bf16_backbone_every_slot_per_image(size):
    """TXO_BACKBONE_BF16=1 against the float64 run that rounds what that mode stores as bf16: close to the emulation, closer by far than
    either sits to the plain float64 result -- per image"""
    cpu_ref = oracle()
    H, W, n, slots = SIZES[size]
    img_n, enc64_n = reference(size)
    emu_n = ref64.encode(weights()[1], img_n, grid_w=dims().grid, backbone_q=lambda x: cpu_ref.bf16_round(x).to(x.dtype))
    m = engine("bf16bk", size)
    w_emu = 0.0
    for S in slots:
        ids, img, enc64 = batch(size, S)
        emu = emu_n[ids]
        enc = encode(m, img, size)
        rel_q, rel_emu, emu_64 = per_image_rel(enc, enc64), per_image_rel(enc, emu, scale=enc64), per_image_rel(emu, enc64)
        w_emu = max(w_emu, assert_each_image_below(rel_emu, 0.1, size, f"bf16 backbone, {S} slots, vs emulation"))
        assert_each_image_below(rel_emu - 0.5 * rel_q, 0.0, size, f"bf16 backbone, {S} slots, (vs emulation) - 0.5 (vs float64)")
        assert_each_image_below((rel_q - emu_64).abs() - 0.5 * emu_64, 0.0, size, f"bf16 backbone, {S} slots, |engine - emulation| distance to float64")
        assert_copies_bit_identical(enc, ids, size, f"bf16 backbone, {S} slots")       # (statistics from gn_partial_kernel: per image)
    print(f"\nhybrid {size} bf16 backbone, worst image over slots {slots}: vs emulation {w_emu:.4f} (bound 0.1); emulation vs float64 "
          f"{float(per_image_rel(emu_n, enc64_n).max()):.4f}")


@pytest.mark.parametrize("kind", ["fp32", "bf16"])
def test_max_tokens_below_the_canvas_traded_for_images(kind):
    """max_tokens = 1 + 2 * 16 with max_batch = 64 (the activation buffers are sized by max_tokens, gn_tiles by the canvas): 64 slots of
    32x256 meet the bounds, and an engine sized for the canvas gives the same bits for the slots it holds"""
    size = "32x256"
    m = engine(kind, size, max_batch=64, max_tokens=1 + 2 * 16)
    ids, img, enc64 = batch(size, 64)
    enc = encode(m, img, size)
    if kind == "fp32":
        assert_each_image_below((enc.double() - enc64).abs().amax(dim=(1, 2)), fp32_bound(size), size, "fp32, max_tokens 33")
    else:
        assert_each_image_below(per_image_rel(enc, enc64), BF16_BOUND, size, "bf16 default, max_tokens 33")
    m_canvas = engine(kind, size, max_batch=5, max_tokens=0)
    assert torch.equal(encode(m_canvas, img[:5], size), enc[:5])


def test_image_chunks_of_7_at_33_slots():
    """TXO_ENC_CHUNK=7 with the hybrid embedder (chunks of 7, 7, 7, 7, 5 images): fp32 bit-identical to the unchunked engine; in the
    default bf16 engine a chunk restarts b at 0, so `split` changes: held to the per-image bounds"""
    size, S = "48x176", 33
    ids, img, enc64 = batch(size, S)
    chunk = {"TXO_ENC_CHUNK": "7"}
    whole32, chunk32 = encode(engine("fp32", size), img, size), encode(engine("fp32", size, env=chunk), img, size)
    assert torch.equal(whole32, chunk32)
    assert_each_image_below((chunk32.double() - enc64).abs().amax(dim=(1, 2)), fp32_bound(size), size, "fp32, chunks of 7")
    whole, chunked = encode(engine("bf16", size), img, size), encode(engine("bf16", size, env=chunk), img, size)
    exact = encode(engine("exact", size, env=chunk), img, size)
    w64 = assert_each_image_below(per_image_rel(chunked, enc64), BF16_BOUND, size, "bf16 default, chunks of 7, vs float64")
    wab = assert_each_image_below(per_image_rel(chunked, exact, scale=enc64), SPLIT_VS_EXACT_BOUND, size,
                                  "bf16 default vs exact backbone, chunks of 7")
    wcw = assert_each_image_below(per_image_rel(chunked, whole, scale=enc64), BF16_BOUND, size,
                                  "bf16 default, chunks of 7 vs whole batch")
    assert_copies_bit_identical(exact, ids, size, "bf16 exact backbone, chunks of 7")
    print(f"\nhybrid {size} chunks of 7, {S} slots, bf16 default, worst image: vs float64 {w64:.5f}, vs exact {wab:.5f}, vs whole batch {wcw:.5f}")


def test_tile_sums_left_by_an_earlier_encode_are_not_read():
    """gn_tiles is one buffer for every convolution of every encode.  After 64 slots of 48x176 tile 48 holds the sums of a stage-1
    tile that straddles two images (48 * 128 mod 132 = 72).  Three slots of 32x256 then end their stem exactly at tile 48
    (3 * 2048 / 128): a finish kernel that walks one tile past an image that ends on a tile seam adds those sums to the last image.
    The encode must give the bits of an engine that has seen nothing else."""
    assert 48 * GB_BM % 132 + GB_BM > 132 and 3 * 2048 == 48 * GB_BM
    m = engine("bf16", "48x176")                                    # 34 tokens: fits 32x256 (33) as well
    encode(m, batch("48x176", 64)[1], "48x176")
    ids, img, enc64 = batch("32x256", 3)
    after = encode(m, img, "32x256")
    fresh = encode(engine("bf16", "32x256"), img, "32x256")
    assert_each_image_below(per_image_rel(after, enc64), BF16_BOUND, "32x256", "bf16 default, 3 slots after 64 of 48x176, vs float64")
    for b in range(3):
        assert torch.equal(after[b], fresh[b]), f"an earlier encode changed the result: {float((after[b] - fresh[b]).abs().max()):.3e}; {where('32x256', b)}"


def test_generate_at_17_slots_fp32():
    """generate() behind the hybrid front end: 12 greedy steps, tokens exact against the float64 oracle up to its first narrow margin,
    and every slot's tokens equal to its copies'"""
    size, S, steps = "48x176", 17, 12
    d = dims()
    ids, img, enc64 = batch(size, S)
    ref_t, ref_l = ref64.generate(weights()[1], reference(size)[1], d.bos, d.eos, steps)
    toks = engine("fp32", size).generate(img, steps).cpu()
    assert toks.shape == (S, ref_t.shape[1])
    assert_tokens_exact_up_to_margin(toks.numpy(), ref_t[ids].numpy(), ref_l[ids])
    for a, b in copies_of(ids):
        assert torch.equal(toks[a], toks[b]), f"slots {a} and {b} hold the same image: {toks[a].tolist()} / {toks[b].tolist()}; {where(size, b)}"
