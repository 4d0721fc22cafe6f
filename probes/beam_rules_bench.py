"""Cost of the constrained beam search (csrc/beam_rules.h; profiles/beam_rules_cost.txt) at the bench's beam shape:
128 images of 3x224x672, k = 5, vocabulary 1000, bf16, 256 positions, eos off so that every position runs.

Three variants of model.beam_search in ONE process, in rounds (so that drift shows as a difference between rounds, not between variants):
  (a) switch off, no rules     -- the parent commit's search: the same kernels, byte for byte (profiles/beam_rules_resource_usage.txt);
  (b) switch on,  no rules     -- must run those same kernels: it has to sit inside (a)'s round-to-round spread;
  (c) switch on,  brace rules  -- rules.brace_rules of the 1k vocabulary fixture, installed once outside the timed calls.

  python probes/beam_rules_bench.py [--images 128] [--beams 5] [--reps 7] [--rounds 3] [--steps 256]
one line per (round, variant): median and spread (min .. max) of the reps, then the medians of the rounds' medians and (c) - (a)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from texocr_amd import rules as R, synth                            # noqa: E402
from texocr_amd.config import Dims                                  # noqa: E402
from texocr_amd.model import model_from_dims                        # noqa: E402
from texocr_amd.tokenizer import RegExTokenizer                     # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--beams", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=256)
    a = ap.parse_args()
    d = Dims(canvas=896)                                            # the bench's beam engine (bench.py: beam_measurement), its 224x672 bucket
    v = json.load(open(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab_1k.json")))
    tk = RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"])
    rules = R.brace_rules(tk, depth_max=64, vocab=d.vocab, eos=d.eos, ban=(d.bos, d.pad)).validate(d.vocab)
    m = model_from_dims(d, dtype="bf16", max_batch=a.images * a.beams, max_tokens=d.n_tokens(224, 896))
    m.load_state_dict(synth.synth_state_dict(d, 0))
    m.eos_token = None
    g = torch.Generator(device="cuda").manual_seed(977)
    img = torch.rand((a.images, d.in_channels, 224, 672), generator=g, device="cuda", dtype=torch.float32)
    eng = m._engine
    variants = [("a: switch off, no rules", False, None), ("b: switch on,  no rules", True, None), ("c: switch on,  brace rules", True, rules)]
    med = {name: [] for name, _, _ in variants}
    for rnd in range(a.rounds):
        for name, on, rs in variants:
            m.rules_beam = on
            eng.set_token_rules(rs)                                 # installed once, outside the timed calls (what a server does)
            mid, lo, hi = timed(lambda: eng.beam_search(img, a.beams, a.steps, None), a.reps)
            med[name].append(mid)
            print(f"round {rnd} {name:27s}: median {mid:7.2f} ms  (min {lo:7.2f} .. max {hi:7.2f}, {a.reps} calls of {a.images} images x {a.beams} beams "
                  f"x {a.steps} positions)", flush=True)
        eng.set_token_rules(None)
    m.rules_beam = False
    mm = {name: statistics.median(x) for name, x in med.items()}
    (na, _, _), (nb, _, _), (nc, _, _) = variants
    spread = max(med[na]) - min(med[na])
    print(f"medians of the rounds: a {mm[na]:.2f} ms (rounds differ by {spread:.2f} ms), b {mm[nb]:.2f} ms (b - a {mm[nb] - mm[na]:+.2f}), "
          f"c {mm[nc]:.2f} ms (c - a {mm[nc] - mm[na]:+.2f} ms, {100 * (mm[nc] - mm[na]) / mm[na]:+.2f} %; "
          f"{1e3 * (mm[nc] - mm[na]) / a.steps:+.2f} us per position)")


if __name__ == "__main__":
    main()
