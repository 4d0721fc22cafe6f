#!/usr/bin/env python3
"""Captures the teacher-forced scoring fixtures tests/golden/score_*.{json,npz} from the imported reference (needs the reference
tree, like oracle/capture_golden.py, whose build_reference it uses; run once where that tree exists, never by the tests).

Per case the reference's own ``loss, out = model.decoder(trg, enc=model.encoder(src), mask=mask, return_out=True)``
(model/decoder.py:124-145) is reduced to what the scoring tests compare: the scalar loss and, per position, log_softmax(out) at the
target, the arg-max, its log-probability and the top-1 / top-2 logit margin.  The logits themselves are not stored.

Usage:  python tests/capture_score_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.capture_golden import TINY, build_reference, save          # noqa: E402  (imports the reference)
from texocr_amd import synth                                           # noqa: E402
from texocr_amd.config import Dims                                     # noqa: E402


def random_trg(d: Dims, rows: int, L: int, seed: int, lengths=None) -> np.ndarray:
    """bos, then ordinary tokens (never bos / eos / pad); a row of `lengths` is cut to its length and padded with d.pad"""
    special = {d.bos, d.eos, d.pad}
    ordinary = np.array([v for v in range(d.vocab) if v not in special])
    rng = np.random.default_rng(seed)
    trg = ordinary[rng.integers(0, len(ordinary), size=(rows, L))]
    trg[:, 0] = d.bos
    for r, n in enumerate(lengths or []):
        trg[r, n - 1] = d.eos
        trg[r, n:] = d.pad
    return trg.astype(np.int64)


@torch.no_grad()
def capture(name: str, d: Dims, weight_seed: int, image_shape, image_seed: int, L: int, trg_seed: int, lengths=None, note: str = ""):
    model, _ = build_reference(d, weight_seed)
    src = torch.from_numpy(synth.synth_images(*image_shape, image_seed))
    trg = torch.from_numpy(random_trg(d, image_shape[0], L, trg_seed, lengths))
    mask = model.make_trg_mask(trg)                                     # ocr_model.py:34-36
    loss, out = model.decoder(trg, enc=model.encoder(src), mask=mask, return_out=True)
    assert float(loss) == float(model(src, trg)), "OCRModel.forward is the same call"
    lsm = torch.log_softmax(out, dim=-1)
    top2 = out.topk(2, dim=-1).values
    top1 = out.argmax(-1)
    save(name, {"dims": d.to_dict(), "weight_seed": weight_seed, "image_seed": image_seed, "image_shape": list(image_shape), "L": L,
                "trg_seed": trg_seed, "padded": bool(lengths), "loss": float(loss), "note": note},
         trg=trg.numpy().astype(np.int16), mask=mask.numpy().astype(np.uint8),
         logp=lsm.gather(-1, trg[:, 1:, None])[..., 0].numpy(), top1=top1.numpy().astype(np.int16),
         top1_logp=lsm.gather(-1, top1[..., None])[..., 0].numpy(), margin=(top2[..., 0] - top2[..., 1]).numpy().astype(np.float32))


if __name__ == "__main__":
    capture("score_tiny", TINY, 7, (2, 3, 32, 48), 11, 13, 21, note="(a) tiny dims, no padding: loss is comparable")
    capture("score_cfg1", Dims(canvas=224), 0, (4, 3, 224, 224), 1234, 33, 22,
            note="(b) config.yml dims, 4 images, L = 33, no padding: loss is comparable")
    capture("score_ragged", TINY, 7, (3, 3, 32, 48), 12, 12, 23, lengths=[12, 7, 4],
            note="(c) rows of 12 / 7 / 4 tokens padded with trg_pad_idx, mask of make_trg_mask; arrays are meaningful only where "
                 "mask[:, :-1] & mask[:, 1:]; loss averages over padded positions as well (no ignore_index) and is not comparable")
