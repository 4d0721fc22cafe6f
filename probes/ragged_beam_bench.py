"""Beam search on a mixed-size batch: one ragged chunk against exact-size buckets.

A seeded mix of 128 images, uniform over the admissible sizes of the 224x672 canvas (14 x 42 of them), the benchmark's model in bf16,
k = 5 beams (640 decode rows), max_len 256, no eos (every search runs its 256 positions).  Measured alternating in ONE process, median:
  (a) OCRModel.beam_search over the list -- ONE ragged encode and ONE decode;
  (b) dist.generate_bucketed over the same list on the same engine -- groups of identical (H, W), one generate(beam=5) each: the only
      route before the ragged call;
  (c) the fixed-shape beam_search at the full canvas, 128 images: the ceiling.
Also prints the share of the B * Ns rows of the ragged chunk that are padding.

    python probes/ragged_beam_bench.py [--images 128] [--beams 5] [--reps 5] [--max-len 256]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from texocr_amd import dist, synth
from texocr_amd.config import Dims
from texocr_amd.model import model_from_dims


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--beams", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-len", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    d = Dims(canvas=224, canvas_w=672)
    m = model_from_dims(d, dtype="bf16", max_batch=a.images * a.beams)
    m.load_state_dict(synth.synth_state_dict(d, 0))
    m.eos_token = None
    rng = np.random.RandomState(a.seed)
    sizes = [(16 * int(rng.randint(1, 15)), 16 * int(rng.randint(1, 43))) for _ in range(a.images)]
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    images = [torch.rand((3, h, w), generator=gen, device="cuda") for h, w in sizes]
    full = torch.rand((a.images, 3, 224, 672), generator=gen, device="cuda")
    ntok = [1 + (h // 16) * (w // 16) for h, w in sizes]
    routes = {
        "(a) beam_search, one ragged chunk": lambda: m.beam_search(images, a.beams, a.max_len),
        "(b) generate_bucketed (exact-size groups)": lambda: dist.generate_bucketed(lambda x: m.generate(x, a.max_len, beam=a.beams), images,
                                                                                     max_batch=a.images),
        "(c) fixed-shape beam_search, full canvas": lambda: m.beam_search(full, a.beams, a.max_len),
    }
    times = {k: [] for k in routes}
    for f in routes.values():                                  # warm-up: stream tuning, caches
        f()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, f in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    groups = len(set(sizes))
    print(f"mix: {a.images} images, {groups} distinct sizes (groups of {a.images / groups:.2f} images on average), tokens per image "
          f"{min(ntok)} .. {max(ntok)}, mean {sum(ntok) / len(ntok):.1f}; bf16, {a.beams} beams, max_len {a.max_len}, no eos; median of {a.reps}")
    print(f"padding share of the B * Ns rows of the ragged chunk: {1 - sum(ntok) / (len(ntok) * max(ntok)):.3f}")
    print(f"{'route':46s} {'ms':>10s} {'images/s':>10s}")
    for k, v in times.items():
        med = statistics.median(v)
        print(f"{k:46s} {med * 1e3:10.1f} {a.images / med:10.1f}   (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f})")


if __name__ == "__main__":
    main()
