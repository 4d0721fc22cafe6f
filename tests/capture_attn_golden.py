#!/usr/bin/env python3
"""Captures the attention-map fixtures tests/golden/attn_*.{json,npz} from the imported reference (needs the reference tree, like
oracle/capture_golden.py, whose build_reference it uses; run once where that tree exists, never by the tests).

Per case the reference's own ``logits, maps = model.decoder.net(x, enc=model.encoder(src), mask=mask, return_attn=True)``
(model/decoder.py:41-67): the post-softmax attention of every block in stack order (self 0, cross 0, self 1, cross 1, ...), each
(B, heads, t, keys) float32, stored in full together with the tokens and the mask.

Usage:  python tests/capture_attn_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.capture_golden import TINY, build_reference, save          # noqa: E402  (imports the reference)
from tests.capture_score_golden import random_trg                      # noqa: E402
from texocr_amd import synth                                           # noqa: E402
from texocr_amd.config import Dims                                     # noqa: E402


@torch.no_grad()
def capture(name: str, d: Dims, weight_seed: int, image_shape, image_seed: int, t: int, trg_seed: int, lengths=None, note: str = ""):
    model, _ = build_reference(d, weight_seed)
    src = torch.from_numpy(synth.synth_images(*image_shape, image_seed))
    x = torch.from_numpy(random_trg(d, image_shape[0], t, trg_seed, lengths))
    mask = model.make_trg_mask(x)                                       # ocr_model.py:34-36
    logits, maps = model.decoder.net(x, enc=model.encoder(src), mask=mask, return_attn=True)
    assert len(maps) == 2 * d.dec_layers
    assert torch.equal(logits, model.decoder.net(x, enc=model.encoder(src), mask=mask)), "return_attn does not change the logits"
    save(name, {"dims": d.to_dict(), "weight_seed": weight_seed, "image_seed": image_seed, "image_shape": list(image_shape), "t": t,
                "trg_seed": trg_seed, "padded": bool(lengths), "note": note},
         x=x.numpy().astype(np.int16), mask=mask.numpy().astype(np.uint8),
         **{f"map{i}": m.numpy().astype(np.float32) for i, m in enumerate(maps)})


if __name__ == "__main__":
    capture("attn_tiny", TINY, 7, (2, 3, 32, 48), 11, 12, 31, note="tiny dims, 2 x 3x32x48 (N = 7), t = 12, no padding")
    capture("attn_pad", TINY, 7, (3, 3, 32, 48), 12, 12, 33, lengths=[12, 7, 4],
            note="rows of 12 / 7 / 4 tokens padded with trg_pad_idx, mask of make_trg_mask; maps are meaningful only at queries that are "
                 "not padding (the reference softmaxes a padded query uniformly over all keys)")
