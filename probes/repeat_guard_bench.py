"""Cost of the repeat guard (txo_set_repeat_guard; csrc/step_guard.h; profiles/repeat_guard_cost.txt) at the headline
constrained shape: 64 images of 3x224x672, config.yml dims, vocabulary 1000, bf16, 256 positions, greedy and sampled, guard (4, 3), without
rules and under rules.brace_rules of the 1k vocabulary fixture.

Per shape two variants in ONE process, interleaved in rounds (drift shows between rounds, not between variants): the same call on the
launch path (TXO_PERSIST=0) with the guard off -- the parent's kernels -- and with the guard set.  Guard and rules are installed outside the
timed calls.

  TXO_PERSIST=0 python probes/repeat_guard_bench.py [--reps 7] [--rounds 3] [--steps 256] [--guard 4 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("TXO_PERSIST", "0")
from texocr_amd import guard, rules as R, synth                     # noqa: E402
from texocr_amd._lib import Q_LAST_GUARDED, Q_LAST_PERSISTENT       # noqa: E402
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


def compare(name, eng, grd, call, a):
    """rounds of (guard off, guard on) -> prints every round and the medians of the rounds' medians"""
    med = {False: [], True: []}
    for rnd in range(a.rounds):
        for on in (False, True):
            eng.set_repeat_guard(grd if on else None)
            mid, lo, hi = timed(call, a.reps)
            assert eng.query(Q_LAST_GUARDED) == int(on) and eng.query(Q_LAST_PERSISTENT) == 0
            med[on].append(mid)
            print(f"{name} round {rnd} {'guard' if on else 'off  '}: median {mid:7.2f} ms  (min {lo:7.2f} .. max {hi:7.2f}, {a.reps} calls)", flush=True)
    eng.set_repeat_guard(None)
    p, c = statistics.median(med[False]), statistics.median(med[True])
    print(f"{name}: off {p:.2f} ms (rounds differ by {max(med[False]) - min(med[False]):.2f} ms), guard {c:.2f} ms (rounds differ by "
          f"{max(med[True]) - min(med[True]):.2f} ms): guard - off {c - p:+.2f} ms = {100 * (c - p) / p:+.2f} %", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--guard", type=int, nargs=2, default=(4, 3))
    a = ap.parse_args()
    grd = tuple(a.guard)
    v = json.load(open(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab_1k.json")))
    tk = RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"])
    g = torch.Generator(device="cuda").manual_seed(977)
    d = Dims(canvas=672)
    brace = R.brace_rules(tk, depth_max=64, vocab=d.vocab, eos=d.eos, ban=(d.bos, d.pad)).validate(d.vocab)
    m = model_from_dims(d, dtype="bf16", max_batch=64)
    m.load_state_dict(synth.synth_state_dict(d, 0))
    eng = m._engine
    img = torch.rand((64, d.in_channels, 224, 672), generator=g, device="cuda", dtype=torch.float32)
    call = lambda: eng.generate(img, a.steps, None)                 # noqa: E731  (no eos: every position runs in every variant)
    free = call().cpu().numpy()
    eng.set_repeat_guard(grd)
    held = call().cpu().numpy()
    eng.set_repeat_guard(None)
    print(f"guard {grd}: the free greedy rows complete a banned block {sum(len(x) for x in guard.violations(free, *grd))} times in {free.size} picks, "
          f"the guarded rows {sum(len(x) for x in guard.violations(held, *grd))} times", flush=True)
    for rules, tag in ((None, "no rules"), (brace, "brace rules")):
        eng.set_token_rules(rules)
        compare(f"greedy  64 x {a.steps}, {tag}", eng, grd, call, a)
        eng.set_sampling(True, temp=0.3, seed=5)
        compare(f"sampled 64 x {a.steps}, {tag}", eng, grd, call, a)
        eng.set_sampling(False)
    eng.set_token_rules(None)


if __name__ == "__main__":
    main()
