"""Ragged batches on the hybrid ResNetV2 front end against the two alternatives (profiles/ragged_hybrid_cost.txt).

The default-factory model (create_model(config.yml): ResNetV2 backbone, 1 x 160 x 1008 canvas, 631 tokens) in bf16, 64 images whose sizes
are uniform over the canvas's admissible sizes (10 x 63 of them), seeded.  Greedy, max_len 256, no eos.  Three routes, alternating in ONE
process after a warm-up of each, median of --reps, wall clock around work that ends in a device synchronise:
  (a) one ragged chunk of 64 (engine.ragged_hybrid = True): container layout, so the padding of the batch's bounding box is computed too;
  (b) exact-size buckets through the fixed-shape call (dist.generate_bucketed): the only correct route without the ragged form -- padding
      to a common size changes the answer, every GroupNorm averages over the padded pixels;
  (c) 64 full-canvas images through the fixed-shape call: the ceiling.
Each is timed for generate() and for the encoder alone.  Prints (a)/(b), (a)/(c) and the share of the container's pixels and of the B * Ns
encoder rows that are padding.  Before timing, the ragged encoder rows of eight images are held against their solo runs (the projection's
256-wide epilogue form is the one this model takes, not the one the small test model does).

    python probes/ragged_hybrid_bench.py [--images 64] [--reps 7] [--max-len 256]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from texocr_amd import dist, synth
from texocr_amd.config import Dims, reference_config
from texocr_amd.model import model_from_dims


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-len", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    d = Dims.from_config(reference_config())
    H, W = d.canvas_hw
    m = model_from_dims(d, dtype="bf16", max_batch=a.images)
    m.load_state_dict(synth.synth_state_dict(d, 0))
    m.eos_token = None
    m.ragged_hybrid = True
    rng = np.random.RandomState(a.seed)
    sizes = [(16 * int(rng.randint(1, H // 16 + 1)), 16 * int(rng.randint(1, W // 16 + 1))) for _ in range(a.images)]
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    images = [torch.rand((1, h, w), generator=gen, device="cuda") for h, w in sizes]
    full = torch.rand((a.images, 1, H, W), generator=gen, device="cuda")
    ntok = [1 + (h // 16) * (w // 16) for h, w in sizes]
    Hb, Wb = max(h for h, _ in sizes), max(w for _, w in sizes)

    # ---- the rows first: ragged against solo, per image relative (tests/gpu_harness.py: per_image_rel)
    enc, nt = m.encoder.forward_ragged(images)
    assert nt.tolist() == ntok and bool(torch.isfinite(enc).all())
    worst = 0.0
    for b in sorted(range(a.images), key=lambda i: ntok[i])[:: max(1, a.images // 8)]:
        solo = m.encoder(images[b][None])[0].double()
        got = enc[b, :ntok[b]].double()
        assert bool((enc[b, ntok[b]:] == 0).all())
        worst = max(worst, float((got - solo).abs().mean() / solo.abs().mean()))
    print(f"ragged encoder rows against the solo run (fused statistics there), worst of the sampled images: {worst:.5f} per image, relative")
    assert worst < 0.02

    def bucketed_encode():
        groups = {}
        for i, s in enumerate(sizes):
            groups.setdefault(s, []).append(i)
        return [m.encoder(torch.stack([images[i] for i in idx])) for idx in groups.values()]

    routes = {
        "generate (a) one ragged chunk": lambda: m.generate_ragged(images, a.max_len),
        "generate (b) exact-size buckets": lambda: dist.generate_bucketed(lambda x: m.generate(x, a.max_len), images, max_batch=a.images),
        "generate (c) full canvas, fixed shape": lambda: m.generate(full, a.max_len),
        "encode   (a) one ragged chunk": lambda: m.encoder.forward_ragged(images),
        "encode   (b) exact-size buckets": bucketed_encode,
        "encode   (c) full canvas, fixed shape": lambda: m.encoder(full),
    }
    times = {k: [] for k in routes}
    for f in routes.values():                                  # warm-up: code objects, captured steps, caches
        f()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, f in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    print(f"mix: {a.images} images, {len(set(sizes))} distinct sizes, tokens per image {min(ntok)} .. {max(ntok)}, mean {sum(ntok) / len(ntok):.1f}; "
          f"bounding box {Hb}x{Wb}; bf16, greedy, max_len {a.max_len}, no eos; median of {a.reps}")
    print(f"padding share of the container's pixels (B * {Hb} * {Wb}): {1 - sum(h * w for h, w in sizes) / (a.images * Hb * Wb):.3f}; "
          f"of the B * Ns encoder rows: {1 - sum(ntok) / (a.images * max(ntok)):.3f}")
    print(f"{'route':42s} {'ms':>10s} {'images/s':>10s}")
    med = {}
    for k, v in times.items():
        med[k] = statistics.median(v)
        print(f"{k:42s} {med[k] * 1e3:10.1f} {a.images / med[k]:10.1f}   (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f})")
    for what in ("generate", "encode  "):
        ra, rb, rc = (med[k] for k in routes if k.startswith(what))
        print(f"{what.strip()}: images/s (a)/(b) = {rb / ra:.2f}, (a)/(c) = {rc / ra:.3f}")


if __name__ == "__main__":
    main()
