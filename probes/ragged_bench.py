"""Ragged batches against exact-size buckets on a realistic mix of image sizes (profiles/ragged_vs_bucketed.txt).

A seeded mix of 256 images, uniform over the admissible sizes of the 224x672 canvas (14 x 42 of them), the benchmark's model in bf16,
greedy, max_len 256, no eos (every decode runs its 256 positions).  Measured alternating in ONE process, median of 7:
  (a) dist.generate_bucketed over the mix -- groups of identical (H, W), one generate() each: the only route before ragged batches;
  (b) generate_ragged in chunks of 64 and of 256;
  (c) the fixed-shape generate at the full canvas, 256 images: the ceiling.
Also prints the share of the B * Ns rows of each ragged chunking that are padding.

    python probes/ragged_bench.py [--images 256] [--reps 7] [--max-len 256]"""
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
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-len", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    d = Dims(canvas=224, canvas_w=672)
    m = model_from_dims(d, dtype="bf16", max_batch=256)
    m.load_state_dict(synth.synth_state_dict(d, 0))
    m.eos_token = None
    rng = np.random.RandomState(a.seed)
    sizes = [(16 * int(rng.randint(1, 15)), 16 * int(rng.randint(1, 43))) for _ in range(a.images)]
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    images = [torch.rand((3, h, w), generator=gen, device="cuda") for h, w in sizes]
    full = torch.rand((a.images, 3, 224, 672), generator=gen, device="cuda")
    ntok = [1 + (h // 16) * (w // 16) for h, w in sizes]

    def ragged(chunk):
        return lambda: [m.generate_ragged(images[i:i + chunk], a.max_len) for i in range(0, a.images, chunk)]

    routes = {
        "(a) generate_bucketed (exact-size groups)": lambda: dist.generate_bucketed(lambda x: m.generate(x, a.max_len), images, max_batch=256),
        "(b) generate_ragged, chunks of 64": ragged(64),
        "(b) generate_ragged, chunks of 256": ragged(256),
        "(c) fixed-shape generate, full canvas": lambda: m.generate(full, a.max_len),
    }
    times = {k: [] for k in routes}
    for k, f in routes.items():                                # warm-up: graphs, tuning, caches
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
    print(f"mix: {a.images} images, {groups} distinct sizes (groups of {a.images / groups:.2f} images on average), "
          f"tokens per image {min(ntok)} .. {max(ntok)}, mean {sum(ntok) / len(ntok):.1f}; bf16, greedy, max_len {a.max_len}, no eos; median of {a.reps}")
    for chunk in (64, 256):
        rows = valid = 0
        for i in range(0, a.images, chunk):
            part = ntok[i:i + chunk]
            rows, valid = rows + len(part) * max(part), valid + sum(part)
        print(f"padding share of the B * Ns rows, chunks of {chunk}: {1 - valid / rows:.3f}")
    print(f"{'route':46s} {'ms':>10s} {'images/s':>10s}")
    for k, v in times.items():
        med = statistics.median(v)
        print(f"{k:46s} {med * 1e3:10.1f} {a.images / med:10.1f}   (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f})")


if __name__ == "__main__":
    main()
