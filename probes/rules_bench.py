"""Cost of the constrained decode at the headline shape (B = 64, 3x224x672, config.yml dims, 256 positions, bf16): generate() under
rules.brace_rules of the 1k vocabulary (launch path: the rules leave the persistent launch) against the same generate() without rules on the
launch path (TXO_PERSIST=0; the plain step kernels are the parent commit's, byte for byte: profiles/step_rules_resource_usage.txt) and,
for scale, against the default path (the persistent launch).  Greedy and sampled.

  python probes/rules_bench.py [--batch 64] [--reps 7]          # one line per (decode, variant): median and spread (min .. max) of the reps
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python probes/rules_bench.py --reps 2 --kernels
                                                               # a run of its own: the step kernels' durations from the trace's statistics

Run it in several fresh processes: the spread between processes is the yardstick the difference is read against (profiles/rules_cost.txt)."""
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
from texocr_amd._lib import Q_LAST_PERSISTENT                       # noqa: E402
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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--kernels", action="store_true", help="launch path only, rules off then on: for a kernel trace")
    a = ap.parse_args()
    d = Dims(canvas=672)
    v = json.load(open(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab_1k.json")))
    tk = RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"])
    rules = R.brace_rules(tk, depth_max=64, vocab=d.vocab, eos=d.eos, ban=(d.bos, d.pad)).validate(d.vocab)
    m = model_from_dims(d, dtype="bf16", max_batch=a.batch)
    m.load_state_dict(synth.synth_state_dict(d, 0))
    m.eos_token = None
    img = torch.from_numpy(synth.synth_images(a.batch, 3, 224, 672, seed=1)).cuda()
    eng = m._engine
    for decode in ("greedy", "sample"):
        kw = dict(decode=decode, temp=0.3, seed=1)
        variants = []
        if not a.kernels:
            variants.append(("default path, no rules", None, None))
        variants += [("launch path, no rules", "0", None), ("launch path, brace rules", "0", rules)]
        for name, persist, rs in variants:
            if persist is None:
                os.environ.pop("TXO_PERSIST", None)
            else:
                os.environ["TXO_PERSIST"] = persist
            # the rule set is installed once, outside the timed calls (what a server does); rules= per call adds one 8 KB upload
            eng.set_token_rules(rs)
            med, lo, hi = timed(lambda: m.generate(img, a.steps, **kw), a.reps)
            path = "persistent" if eng.query(Q_LAST_PERSISTENT) else "launches"
            print(f"batch {a.batch} {decode:6s} {name:26s} ({path:10s}): median {med:7.2f} ms  (min {lo:7.2f} .. max {hi:7.2f}, {a.reps} calls)", flush=True)
        eng.set_token_rules(None)


if __name__ == "__main__":
    main()
