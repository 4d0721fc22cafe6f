"""Ragged batches on the hybrid ResNetV2 front end, the part that needs no GPU.

1. One low-side SAME offset per layer serves a batch of mixed sizes: for every side that is a multiple of 16 up to the canvas's, the
   rule of Engine::same_pad (csrc/engine.hip), restated in hybrid_ragged_ref.same_pad_low, gives the constant of the table
       stem 7x7/2 on H: 2    max pool 3x3/2 on H/2: 0    3x3/1: 1    3x3/2 on an even side: 0    1x1/2: 0
   at every resolution the backbone meets the layer at.
2. The container algorithm (tests/hybrid_ragged_ref.py: masked taps, GroupNorm over the extent, token packing, everything outside an extent
   overwritten with NaN between layers) against oracle/cpu_ref.py on each image alone, in float64.  The two differ only in the order of
   float64 sums (another tensor shape takes another blocking inside conv2d): float64 rounding, 1.1e-16, through 45 layers that amplify a
   relative perturbation by less than 1e3 (tests/test_gpu_hybrid.py: 2^-17 per product arrives as 7e-3) stays below 1e-12 of the largest value.
"""
import functools

import pytest
import torch

import hybrid_ragged_ref as hr
import ref64
from oracle import cpu_ref
from texocr_amd import synth
from texocr_amd.config import Dims

CANVAS = (160, 1008)
DIMS = Dims(canvas=CANVAS[0], canvas_w=CANVAS[1], embed="hybrid", in_channels=1, embed_dim=64, enc_heads=1, enc_layers=1, dec_heads=1,
            dec_layers=1, vocab=32, max_len=8, bos=30, eos=29, pad=31)
SIZES = [(64, 320), (16, 16), (32, 256), (48, 176), (16, 1008)]       # tests/test_gpu_hybrid.py: SIZES; container 64 x 1008
COPIES = {5: 1, 6: 3}                                                 # slot: the slot it repeats
REL_BOUND = 1e-12


def test_one_low_pad_per_layer_for_every_accepted_side():
    for canvas_side in CANVAS:
        for side in range(16, canvas_side + 1, 16):
            assert hr.same_pad_low(side, 7, 2) == 2 == hr.LOW_PAD[(7, 2)], side                       # stem on H
            assert hr.same_pad_low(side // 2, 3, 2) == 0 == hr.POOL_LOW_PAD, side                     # pool on H/2
            for s in (4, 8, 16):                                                                     # the stages' resolutions
                assert hr.same_pad_low(side // s, 3, 1) == 1 == hr.LOW_PAD[(3, 1)], (side, s)
                assert hr.same_pad_low(side // s, 1, 1) == 0 == hr.LOW_PAD[(1, 1)], (side, s)
            for s in (4, 8):                                                                         # the strided first block of stages 1 and 2
                assert (side // s) % 2 == 0
                assert hr.same_pad_low(side // s, 3, 2) == 0 == hr.LOW_PAD[(3, 2)], (side, s)
                assert hr.same_pad_low(side // s, 1, 2) == 0 == hr.LOW_PAD[(1, 2)], (side, s)
    # the rule is not constant off the multiples of 16: what the accepted sizes buy
    assert hr.same_pad_low(15, 7, 2) == 3 and hr.same_pad_low(9, 3, 2) == 1


@functools.lru_cache(maxsize=None)
def case():
    assert DIMS.embed == "hybrid" and DIMS.canvas_hw == CANVAS
    sd = ref64.sd64(synth.synth_state_dict(DIMS, 9))
    images = [torch.from_numpy(synth.synth_images(1, 1, h, w, seed=31 + i))[0].double() for i, (h, w) in enumerate(SIZES)]
    images += [images[COPIES[5]].clone(), images[COPIES[6]].clone()]
    box, sizes = hr.pack(images, 64, 1008)
    assert bool(torch.isnan(box).any())
    return sd, images, box, sizes


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_container_tokens_equal_hybrid_embed_per_image():
    sd, images, box, sizes = case()
    tok, ntok = hr.container_tokens(sd, box, sizes)
    assert tok.dtype == torch.float64 and tok.shape == (7, 4 * 20, DIMS.embed_dim)
    worst = 0.0
    for b, im in enumerate(images):
        solo = cpu_ref.hybrid_embed(sd, im[None])[0]
        assert ntok[b] == 1 + solo.shape[0] and bool(torch.isfinite(tok[b, :ntok[b] - 1]).all())
        worst = max(worst, rel(tok[b, :ntok[b] - 1], solo))
        assert bool((tok[b, ntok[b] - 1:] == 0).all())
    print(f"\ncontainer tokens vs hybrid_embed per image, float64: worst relative difference {worst:.2e} (bound {REL_BOUND:g})")
    assert worst < REL_BOUND
    for slot, first in COPIES.items():
        assert torch.equal(tok[slot], tok[first])


def test_container_encode_equals_encode_per_image():
    sd, images, box, sizes = case()
    enc, ntok = hr.container_encode(sd, box, sizes, DIMS.grid)
    worst = 0.0
    for b, im in enumerate(images):
        solo = ref64.encode(sd, im[None], grid_w=DIMS.grid)[0]
        assert solo.shape == (ntok[b], DIMS.embed_dim)
        worst = max(worst, rel(enc[b, :ntok[b]], solo))
        assert bool((enc[b, ntok[b]:] == 0).all())
    print(f"\ncontainer encode vs encode per image, float64: worst relative difference {worst:.2e} (bound {REL_BOUND:g})")
    assert worst < REL_BOUND


def test_padding_to_a_common_size_is_no_way_round_it():
    """what the container algorithm is for: the same image zero-padded to the container changes its own tokens by far more than rounding"""
    sd, images, _, _ = case()
    im = images[2]                                                     # 32 x 256
    padded = torch.zeros((1, 1, 64, 320), dtype=torch.float64)
    padded[0, :, :32, :256] = im
    solo = cpu_ref.hybrid_embed(sd, im[None])[0].reshape(2, 16, -1)
    pad = cpu_ref.hybrid_embed(sd, padded)[0].reshape(4, 20, -1)[:2, :16]
    assert rel(pad, solo) > 1e-2
