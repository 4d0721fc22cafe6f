"""Cost of the prompted decode at the headline shape (3x224x672, config.yml dims, bf16): decoder.generate(start_tokens of length P) through
the engine's loop (txo_generate_prefix_from_enc) against (a) the stepwise Python loop it replaces (decoder._generate_stepwise: the route
every start other than one BOS column took before) and (b) generate() from BOS over all 256 positions.  prefix + continuation = 256.

  python probes/prefix_bench.py --batch 64 --prefix 1 64 192 [--reps 5]

One line per prefix length: median ms per call of the three, after one warm-up call each.  Throughput at batch 256 varies by process:
run several fresh processes and take the median of their lines (profiles/prefix_cost.txt)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from texocr_amd import synth                                        # noqa: E402
from texocr_amd.config import Dims                                  # noqa: E402
from texocr_amd.model import model_from_dims                        # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--prefix", type=int, nargs="+", default=[1, 64, 192])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--total", type=int, default=256)
    a = ap.parse_args()
    d = Dims(canvas=672)
    m = model_from_dims(d, dtype="bf16", max_batch=a.batch)
    m.load_state_dict(synth.synth_state_dict(d, 0))
    m.eos_token = None
    img = torch.from_numpy(synth.synth_images(a.batch, 3, 224, 672, seed=1)).cuda()
    enc = m.encoder(img)
    bos = torch.full((a.batch, 1), d.bos, dtype=torch.int64, device="cuda")
    full = m.decoder.generate(bos, None, a.total, enc=enc)
    t_bos = timed(lambda: m.decoder.generate(bos, None, a.total, enc=enc), a.reps)
    print(f"batch {a.batch}: generate from BOS over {a.total} positions {t_bos:8.1f} ms", flush=True)
    for P in a.prefix:
        start = torch.cat([bos, full[:, :P - 1]], 1)
        n = a.total - (P - 1)
        if P == 1:
            start = start.clone()
            start[:, 0] = d.bos                                       # (one BOS column takes generate()'s own route: time the prompted one through prefix_len)
            new = lambda: m.decoder.generate(start, None, n, enc=enc, prefix_len=[1] * a.batch)
        else:
            new = lambda: m.decoder.generate(start, None, n, enc=enc)
        t_new = timed(new, a.reps)
        t_old = timed(lambda: m.decoder._generate_stepwise(start, None, n, enc, None), max(1, a.reps // 2))
        print(f"batch {a.batch} prefix {P:3d} (+{n:3d}): prompted loop {t_new:8.1f} ms   stepwise loop {t_old:8.1f} ms   x{t_old / t_new:5.2f}", flush=True)


if __name__ == "__main__":
    main()
