"""Cost of the repeat guard inside beam search (csrc/beam_guard.h; profiles/beam_guard_cost.txt) at the bench's beam shape:
128 images of 3x224x672, k = 5, vocabulary 1000, bf16, 256 positions, guard (4, 3), eos off so that every position runs (the closing
variant needs the model's eos: it runs with it, and its own unguarded twin beside it).

Variants of model.beam_search in ONE process, in rounds (so that drift shows as a difference between rounds, not between variants):
  (a) switch off, no guard            -- the parent commit's search: the same kernels (profiles/beam_guard_resource_usage.txt);
  (b) switch on,  no guard            -- must run those same kernels: it has to sit inside (a)'s round-to-round spread;
  (c) switch on,  guard               -- beam_select_guard_kernel without rules;
  (d) rules only / (e) rules + guard  -- rules.brace_rules of the 1k vocabulary fixture (rules_beam on);
  (f) closing only / (g) closing + guard.

  python probes/beam_guard_bench.py [--images 128] [--beams 5] [--reps 7] [--rounds 3] [--steps 256] [--guard 4 3]
  python probes/beam_guard_bench.py --tree PATH    times variant (a) alone with the package of ANOTHER checkout (the parent commit's, built)
one line per (round, variant): median and spread (min .. max) of the reps, then the medians of the rounds' medians and the differences."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=128)
ap.add_argument("--beams", type=int, default=5)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=256)
ap.add_argument("--guard", type=int, nargs=2, default=(4, 3))
ap.add_argument("--tree", default="")
ARGS = ap.parse_args()
ROOT = os.path.abspath(ARGS.tree) if ARGS.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    a = ARGS
    d = Dims(canvas=896)                                            # the bench's beam engine (bench.py: beam_measurement), its 224x672 bucket
    v = json.load(open(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab_1k.json")))
    tk = RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"])
    rules = R.brace_rules(tk, depth_max=64, vocab=d.vocab, eos=d.eos, ban=(d.bos, d.pad)).validate(d.vocab)
    m = model_from_dims(d, dtype="bf16", max_batch=a.images * a.beams, max_tokens=d.n_tokens(224, 896))
    m.load_state_dict(synth.synth_state_dict(d, 0))
    g = torch.Generator(device="cuda").manual_seed(977)
    img = torch.rand((a.images, d.in_channels, 224, 672), generator=g, device="cuda", dtype=torch.float32)
    eng = m._engine
    guard = tuple(a.guard)
    #           name                           switch guard  rules  close
    variants = [("a: switch off, no guard", False, None, None, False)]
    if not a.tree:
        variants += [("b: switch on,  no guard", True, None, None, False), ("c: switch on,  guard", True, guard, None, False),
                     ("d: brace rules", True, None, rules, False), ("e: brace rules + guard", True, guard, rules, False),
                     ("f: closing", True, None, rules, True), ("g: closing + guard", True, guard, rules, True)]
        m.rules_beam = True
    med = {v_[0]: [] for v_ in variants}
    for rnd in range(a.rounds):
        for name, on, gd, rs, close in variants:
            if not a.tree:
                m.guard_beam = on
            eos = d.eos if close else None                          # (a closing search needs the engine's eos; synthetic weights rarely emit it)
            with eng.modes(rules=rs, close=close, repeat_guard=gd):  # installed once, outside the timed calls (what a server does)
                mid, lo, hi = timed(lambda: eng.beam_search(img, a.beams, a.steps, eos), a.reps)
            med[name].append(mid)
            print(f"round {rnd} {name:27s}: median {mid:7.2f} ms  (min {lo:7.2f} .. max {hi:7.2f}, {a.reps} calls of {a.images} images x {a.beams} beams "
                  f"x {a.steps} positions)", flush=True)
    mm = {name: statistics.median(x) for name, x in med.items()}
    na = variants[0][0]
    print(f"medians of the rounds: {na} {mm[na]:.2f} ms (rounds differ by {max(med[na]) - min(med[na]):.2f} ms)")
    if a.tree:
        return
    m.guard_beam = False
    names = [v_[0] for v_ in variants]
    for name, base in ((names[1], na), (names[2], na), (names[4], names[3]), (names[6], names[5])):
        diff = mm[name] - mm[base]
        print(f"  {name:27s} {mm[name]:7.2f} ms  against {base:27s} {mm[base]:7.2f} ms: {diff:+.2f} ms, {100 * diff / mm[base]:+.2f} %, "
              f"{1e3 * diff / a.steps:+.2f} us per position")


if __name__ == "__main__":
    main()
