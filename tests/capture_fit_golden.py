#!/usr/bin/env python3
"""Captures tests/golden/fit_cases.{npz,json}: the source bytes of the fit-to-canvas cases and what PIL makes of them,
``img.resize((w', h'), Image.BILINEAR)`` with (h', w') by the fit rule and an RGBA image taken through ``convert('RGB')`` first.  With
the fixture the tests need no PIL: tests/fit_ref.py must reproduce every ``out_*`` array, and the GPU tests compare the engine against
fit_ref on the same sources.  Run once where PIL is installed, never by the tests; the PIL version is recorded in the json.

Usage:  python tests/capture_fit_golden.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fit_ref                                                            # noqa: E402

# (name, mode, h, w, (Fh, Fw)): the mixed batch of the container test -- images that fit, and oversized ones: one pixel over on either
# side, an exact x2, odd sizes in RGB / RGBA, one-pixel strips, scale 32 on both axes, a height that clamps to 1
BATCH = [
    ("fits_1x1", "L", 1, 1), ("fits_16x16", "RGBA", 16, 16), ("fits_32x96", "L", 32, 96), ("fits_20x50", "RGB", 20, 50),
    ("over_33x96", "L", 33, 96), ("over_32x97", "RGB", 32, 97), ("over_64x192", "L", 64, 192), ("over_47x301", "RGB", 47, 301),
    ("over_70x500", "RGBA", 70, 500), ("over_1x400", "L", 1, 400), ("over_300x1", "RGB", 300, 1), ("over_1024x3072", "L", 1024, 3072),
    ("over_2x3000", "L", 2, 3000),
]
CH = {"L": 1, "RGB": 3, "RGBA": 4}


def batch_source(name, mode, h, w, rng):
    if name == "over_1024x3072":      # 3 MB of pixels: a pattern zlib folds to a few KB (every byte value; steps of 0 -> 255 across both axes)
        r, c = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        return ((r * 5 + c * 3) % 256 * ((r // 16 + c // 48) % 2) + 255 * ((r // 40 + c // 100) % 3 == 0)).clip(0, 255).astype(np.uint8)
    a = rng.integers(0, 256, (h, w, CH[mode]), dtype=np.uint8)
    return a[..., 0] if mode == "L" else a


def coverage_source():
    """64 x 512 under the target (16, 16) becomes 2 x 16: scale 32 and up to 64 taps on both axes.  Left half: columns alternate 0 and 255,
    the phase flipped every other row, so 0 meets 255 inside every window on both axes; right half: every byte value, the ramp reversed on
    odd rows."""
    a = np.zeros((64, 512), np.uint8)
    r, c = np.meshgrid(np.arange(64), np.arange(256), indexing="ij")
    a[:, :256] = np.where((c + (r // 2)) % 2, 255, 0)
    a[:, 256:] = np.where(r % 2, 255 - c, c)
    return a


def pil_fit(a, Fh, Fw):
    from PIL import Image
    h, w = a.shape[:2]
    fh, fw = fit_ref.fit_size(h, w, Fh, Fw)
    img = Image.fromarray(a)
    if img.mode != "L":
        img = img.convert("RGB")
    return np.asarray(img.resize((fw, fh), Image.BILINEAR))


def main():
    import PIL
    rng = np.random.default_rng(20240607)
    arrays, cases = {}, []

    def add(name, a, Fh, Fw):
        h, w = a.shape[:2]
        fh, fw = fit_ref.fit_size(h, w, Fh, Fw)
        arrays["src_" + name] = a
        if (fh, fw) != (h, w):
            arrays["out_" + name] = pil_fit(a, Fh, Fw)
        cases.append(dict(name=name, mode={2: "L", 3: {3: "RGB", 4: "RGBA"}.get(a.shape[-1])}[a.ndim], h=h, w=w, Fh=Fh, Fw=Fw, fh=fh, fw=fw))

    for name, mode, h, w in BATCH:
        add(name, batch_source(name, mode, h, w, rng), 32, 96)
    add("coverage_64x512", coverage_source(), 16, 16)
    add("white_64x512", np.full((64, 512), 255, np.uint8), 16, 16)
    add("white_rgb_40x130", np.full((40, 130, 3), 255, np.uint8), 16, 16)
    out = os.path.join(ROOT, "tests", "golden")
    np.savez_compressed(os.path.join(out, "fit_cases.npz"), **arrays)
    with open(os.path.join(out, "fit_cases.json"), "w") as f:
        json.dump(dict(pil=PIL.__version__, filter="BILINEAR", note="out_* = PIL's resize of src_* (RGBA through convert('RGB')) to (fh, fw)",
                       cases=cases), f, indent=1)
        f.write("\n")
    print("wrote", len(cases), "cases;", os.path.getsize(os.path.join(out, "fit_cases.npz")), "bytes")


if __name__ == "__main__":
    main()
