"""Cost of alternatives per token (txo_set_alternatives; csrc/step_alts.h; profiles/alts_cost.txt) at the headline shape:
64 images of 3x224x672, config.yml dims, vocabulary 1000, bf16, 256 positions, greedy and sampled, k = 1, 4, 8.

Per decode mode, variants in ONE process, interleaved in rounds (drift shows between rounds, not between variants):
  launch  the launch path (TXO_PERSIST=0) with alternatives off -- against it, k = 1 / 4 / 8 is the new kernel's own cost;
  persist the default path with alternatives off (the persistent launch) -- against it, what leaving that launch costs;
  logits  return_logits=True + log_softmax + topk(8) on the device, the route alternatives replace: time and peak memory.

  python probes/alts_bench.py [--reps 7] [--rounds 3] [--steps 256]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from texocr_amd import synth                                        # noqa: E402
from texocr_amd._lib import Q_LAST_ALTS, Q_LAST_PERSISTENT          # noqa: E402
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
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=256)
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(977)
    d = Dims(canvas=672)
    m = model_from_dims(d, dtype="bf16", max_batch=64)
    m.load_state_dict(synth.synth_state_dict(d, 0))
    eng = m._engine
    img = torch.rand((64, d.in_channels, 224, 672), generator=g, device="cuda", dtype=torch.float32)

    def run(persist, k=0, logits=False):
        os.environ["TXO_PERSIST"] = persist
        eng.query(4)                                                # TXO_Q_RELOAD_KNOBS
        eng.set_alternatives(k)
        if logits:
            tok, lg = eng.generate(img, a.steps, None, return_logits=True)
            return torch.log_softmax(lg, -1).topk(8, dim=-1)
        return eng.generate(img, a.steps, None)                     # (no eos: every position runs in every variant)

    variants = [("launch ", lambda: run("0")), ("k = 1  ", lambda: run("0", 1)), ("k = 4  ", lambda: run("0", 4)), ("k = 8  ", lambda: run("0", 8)),
                ("persist", lambda: run("")), ("logits ", lambda: run("0", logits=True))]
    for mode in ("greedy", "sampled"):
        eng.set_sampling(mode == "sampled", temp=0.3, seed=5)
        med = {n: [] for n, _ in variants}
        for rnd in range(a.rounds):
            for n, call in variants:
                torch.cuda.reset_peak_memory_stats()
                mid, lo, hi = timed(call, a.reps)
                peak = torch.cuda.max_memory_allocated() / 2**20
                med[n].append(mid)
                print(f"{mode} round {rnd} {n}: median {mid:7.2f} ms  (min {lo:7.2f} .. max {hi:7.2f}, {a.reps} calls)  persistent {eng.query(Q_LAST_PERSISTENT)} "
                      f"alts {eng.query(Q_LAST_ALTS)}  torch peak {peak:7.1f} MiB", flush=True)
        base = statistics.median(med["launch "])
        for n, _ in variants:
            c = statistics.median(med[n])
            print(f"{mode} {n}: {c:7.2f} ms (rounds differ by {max(med[n]) - min(med[n]):.2f} ms): - launch {c - base:+.2f} ms = {100 * (c - base) / base:+.2f} %", flush=True)
    eng.set_sampling(False)
    eng.set_alternatives(0)
    os.environ.pop("TXO_PERSIST", None)


if __name__ == "__main__":
    main()
