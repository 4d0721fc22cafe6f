"""Cost of the closing decode (txo_set_rules_close; csrc/step_rules.h, csrc/beam_rules.h; profiles/rules_close_cost.txt)
at the headline constrained shape: 64 images of 3x224x672, config.yml dims, vocabulary 1000, bf16, 256 positions, greedy and sampled, and
the bench's beam shape, 128 images x 5 beams.  rules.brace_rules of the 1k vocabulary fixture (depth_max 64: dist_max 65, so the budgeted
branch can run in the last 65 positions only); eos is the model's own -- a closing decode needs it --, which random weights rarely pick, so
both variants run every position.

Per shape two variants in ONE process, in rounds (drift shows between rounds, not between variants): the same constrained call without
close (the parent's kernels) and with close=True.  Rules and switch are installed once, outside the timed calls.  Also the installation
time of the table for the 1k brace rule set (txo_set_rules_close with the rules set: the host search + one 4 KB copy).

--depth-max 2 leaves the budgeted branch three positions: what close costs then is the slack branch's (the plain masking code behind the
row's two extra words), which tells the two branches apart.

  python probes/rules_close_bench.py [--reps 7] [--rounds 3] [--steps 256] [--skip-beam] [--depth-max 64]"""
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


def compare(name, eng, rules, call, a):
    """rounds of (plain constrained, closing) -> prints every round and the medians of the rounds' medians"""
    med = {False: [], True: []}
    eng.set_token_rules(rules)
    for rnd in range(a.rounds):
        for close in (False, True):
            torch.ops.texocr.set_rules_close(eng.id, close)
            mid, lo, hi = timed(call, a.reps)
            med[close].append(mid)
            print(f"{name} round {rnd} {'close' if close else 'plain'}: median {mid:7.2f} ms  (min {lo:7.2f} .. max {hi:7.2f}, {a.reps} calls)", flush=True)
    torch.ops.texocr.set_rules_close(eng.id, False)
    eng.set_token_rules(None)
    p, c = statistics.median(med[False]), statistics.median(med[True])
    print(f"{name}: plain {p:.2f} ms (rounds differ by {max(med[False]) - min(med[False]):.2f} ms), close {c:.2f} ms (rounds differ by "
          f"{max(med[True]) - min(med[True]):.2f} ms): close - plain {c - p:+.2f} ms = {100 * (c - p) / p:+.2f} %", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--skip-beam", action="store_true")
    ap.add_argument("--depth-max", type=int, default=64, help="the brace rules' depth cap: dist_max = depth_max + 1 positions can run the budgeted branch")
    a = ap.parse_args()
    v = json.load(open(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab_1k.json")))
    tk = RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"])
    g = torch.Generator(device="cuda").manual_seed(977)

    d = Dims(canvas=672)
    rules = R.brace_rules(tk, depth_max=a.depth_max, vocab=d.vocab, eos=d.eos, ban=(d.bos, d.pad)).validate(d.vocab)
    t0 = time.perf_counter()
    dist = rules.close_dist(d.eos)
    print(f"numpy close_dist of the 1k brace rules: {1e3 * (time.perf_counter() - t0):.2f} ms; dist_max {dist.dist_max}, dist[0][0] {int(dist[0, 0])}")
    m = model_from_dims(d, dtype="bf16", max_batch=64)
    m.load_state_dict(synth.synth_state_dict(d, 0))
    eng = m._engine
    img = torch.rand((64, d.in_channels, 224, 672), generator=g, device="cuda", dtype=torch.float32)
    eng.set_token_rules(rules)
    inst = []
    for _ in range(20):
        t0 = time.perf_counter()
        torch.ops.texocr.set_rules_close(eng.id, True)
        inst.append((time.perf_counter() - t0) * 1e3)
        torch.ops.texocr.set_rules_close(eng.id, False)
    print(f"installation of the table (txo_set_rules_close with the 1k brace rules set): median {statistics.median(inst):.3f} ms "
          f"(min {min(inst):.3f} .. max {max(inst):.3f}, 20 calls)", flush=True)
    compare("greedy  64 x 256", eng, rules, lambda: eng.generate(img, a.steps, d.eos), a)
    eng.set_sampling(True, temp=0.3, seed=5)
    compare("sampled 64 x 256", eng, rules, lambda: eng.generate(img, a.steps, d.eos), a)
    eng.set_sampling(False)
    if a.skip_beam:
        return
    del m, eng
    d = Dims(canvas=896)                                            # the bench's beam engine, its 224x672 bucket
    rules = R.brace_rules(tk, depth_max=a.depth_max, vocab=d.vocab, eos=d.eos, ban=(d.bos, d.pad)).validate(d.vocab)
    m = model_from_dims(d, dtype="bf16", max_batch=128 * 5, max_tokens=d.n_tokens(224, 896))
    m.load_state_dict(synth.synth_state_dict(d, 0))
    m.rules_beam = True
    eng = m._engine
    img = torch.rand((128, d.in_channels, 224, 672), generator=g, device="cuda", dtype=torch.float32)
    compare("beam 128 x 5 x 256", eng, rules, lambda: eng.beam_search(img, 5, a.steps, d.eos), a)


if __name__ == "__main__":
    main()
