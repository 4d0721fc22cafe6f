"""Three routes to the confidence of a generate() result, timed at the benchmark shape (224 x 672 images, 256 positions, bf16,
config.yml dims, synthetic weights, no eos: every call decodes all positions):

  logp     generate(return_logp=True)            the token selection's own log-sum-exp (txo_generate_logp)
  logits   generate(return_logits=True)          (B, 256, V) float32 logits, the caller takes log_softmax + gather
  score    generate() + score(img, [bos]+tokens)  a second, teacher-forced pass (txo_score)
  plain    generate()                            the baseline none of them can beat

usage: python probes/logp_routes.py [--batch 64 256] [--reps 5] [--out FILE]
Per batch size: median / min wall time in ms of `reps` calls after 2 warm-up calls (torch.cuda.synchronize around each call), the
decode path the logp route took, and each route's cost over plain."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from texocr_amd import synth
from texocr_amd._lib import Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES
from texocr_amd.config import Dims
from texocr_amd.model import model_from_dims


def timed(fn, reps):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-len", type=int, default=256)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    d = Dims(canvas=224, canvas_w=672)
    sd = synth.synth_state_dict(d, 0)
    lines = []
    for B in a.batch:
        m = model_from_dims(d, dtype=a.dtype, max_batch=B)
        m.load_state_dict(sd)
        m.eos_token = None
        img = torch.from_numpy(synth.synth_images(B, 3, 224, 672, seed=1)).cuda()
        bos = torch.full((B, 1), d.bos, dtype=torch.int64, device="cuda")

        def by_logits():
            t, lg = m.generate(img, a.max_len, return_logits=True)
            return torch.log_softmax(lg, -1).gather(-1, t[..., None])[..., 0]

        def by_score():
            t = m.generate(img, a.max_len)
            return m.score(img, torch.cat([bos, t], 1)).logp

        routes = {"plain": lambda: m.generate(img, a.max_len), "logp": lambda: m.generate(img, a.max_len, return_logp=True),
                  "logits": by_logits, "score": by_score}
        res = {k: timed(f, a.reps) for k, f in routes.items()}
        m.generate(img, a.max_len, return_logp=True)
        path = f"persistent={m._engine.query(Q_LAST_PERSISTENT)} row_ranges={m._engine.query(Q_LAST_ROW_RANGES)}"
        p_logp = m.generate(img, a.max_len, return_logp=True)[1]
        d_logits = float((by_logits() - p_logp).abs().max())
        d_score = float((by_score() - p_logp).abs().max())
        base = res["plain"][0]
        for k, (med, lo) in res.items():
            lines.append(f"batch {B:4d} {a.dtype} {k:7s} median {med:8.2f} ms  min {lo:8.2f} ms  {100 * (med / base - 1):+6.1f} % over plain  {B / med * 1e3:8.1f} images/s")
        lines.append(f"batch {B:4d} logp route: {path}; max |logp - logits route| {d_logits:.2e}, max |logp - score route| {d_score:.2e}")
        del m
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(" ".join(sys.argv) + "\n" + text + "\n")
        print(json.dumps({"wrote": a.out}))


if __name__ == "__main__":
    main()
