"""What teacher-forced scoring of a mixed-size list costs in one ragged chunk against one call per image (DESIGN section 5,
profiles/ragged_forward_cost.txt).

The seeded mix of probes/ragged_bench.py: 256 images, uniform over the admissible sizes of the 224x672 canvas, the benchmark's model in
bf16.  Every image gets a random transcription of L = 65 columns (64 scored positions).  Two routes, each timed as the median of --reps
runs after one warm-up run, with a device synchronisation in front of and behind every run:
  --route ragged   one OCRModel.score_ragged call over all 256 images (one encode, one multi-position decoder pass);
  --route loop     256 calls of OCRModel.score, one image each: the only route before the ragged forward.
The loop uses nothing this route's commit added, so it can be run from a checkout of the parent commit with this file copied in; that is
how the number in profiles/ragged_forward_cost.txt was taken.  `--route both` runs the two alternating in one process and also checks
that the rows agree.

    python probes/ragged_forward_cost.py [--route both] [--images 256] [--reps 7] [--L 65]
TXO_TREE=<another checkout, built>: import texocr_amd from there instead of from this file's tree (the parent-commit run)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.environ.get("TXO_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from texocr_amd import synth
from texocr_amd.config import Dims
from texocr_amd.model import model_from_dims


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=["ragged", "loop", "both"], default="both")
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--L", type=int, default=65)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    d = Dims(canvas=224, canvas_w=672)
    m = model_from_dims(d, dtype="bf16", max_batch=256)
    m.load_state_dict(synth.synth_state_dict(d, 0))
    rng = np.random.RandomState(a.seed)
    sizes = [(16 * int(rng.randint(1, 15)), 16 * int(rng.randint(1, 43))) for _ in range(a.images)]
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    images = [torch.rand((3, h, w), generator=gen, device="cuda") for h, w in sizes]
    ordinary = torch.tensor([v for v in range(d.vocab) if v not in (d.bos, d.eos, d.pad)])
    trg = ordinary[torch.randint(0, len(ordinary), (a.images, a.L), generator=torch.Generator().manual_seed(a.seed))]
    trg[:, 0] = d.bos
    trg = trg.cuda()
    routes = {}
    if a.route in ("ragged", "both"):
        routes["one score_ragged chunk"] = lambda: m.score_ragged(images, trg).logp
    if a.route in ("loop", "both"):
        routes["per-image loop of score"] = lambda: torch.cat([m.score(im[None], trg[b:b + 1]).logp for b, im in enumerate(images)])
    out = {k: f() for k, f in routes.items()}                  # warm-up
    torch.cuda.synchronize()
    times = {k: [] for k in routes}
    for _ in range(a.reps):
        for k, f in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    ntok = [1 + (h // 16) * (w // 16) for h, w in sizes]
    print(f"mix: {a.images} images, {len(set(sizes))} distinct sizes, tokens per image {min(ntok)} .. {max(ntok)}, mean {sum(ntok) / len(ntok):.1f}; "
          f"bf16, L = {a.L} ({a.L - 1} scored positions per image); median of {a.reps}")
    print(f"{'route':28s} {'ms':>10s} {'images/s':>10s}")
    for k, v in times.items():
        med = statistics.median(v)
        print(f"{k:28s} {med * 1e3:10.1f} {a.images / med:10.1f}   (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f})")
    if len(out) == 2:
        x, y = out.values()
        print(f"rows of the two routes bit-identical: {torch.equal(x, y)} (max |d| {float((x - y).abs().max()):.2e})")


if __name__ == "__main__":
    main()
