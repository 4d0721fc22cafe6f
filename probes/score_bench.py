#!/usr/bin/env python3
"""OCRModel.score (fused logits -> log-softmax -> gather, csrc/score.h) against the route that existed before it:
decoder.net(x, enc=enc) -> torch.log_softmax -> gather on the full (B, L-1, V) fp32 logits.

config.yml dims, 3x224x672 images, L = 257; 64 and 256 images; both dtypes.  The two routes alternate inside one process
(same encoder output, same tokens), each timed with device events over whole calls after a warm-up of both; the table gives the
median, the spread, the peak device memory above what is allocated before the call (torch.cuda.max_memory_allocated: torch's
allocations only, which is where the logits and the log-softmax live) and the largest |dlogp| between the two routes.

Usage (GPU box, repository root):  python probes/score_bench.py [out.txt]   (default profiles/score_fused_vs_logits.txt)"""
import datetime
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from texocr_amd.config import Dims                       # noqa: E402
from texocr_amd.model import model_from_dims             # noqa: E402
from texocr_amd import synth                             # noqa: E402

L, REPS, WARM = 257, 7, 2


def timed(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - base, out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "score_fused_vs_logits.txt")
    if not torch.cuda.is_available():
        raise SystemExit("score_bench needs the GPU: nothing is measured without one")
    d = Dims(canvas=672)
    sd = synth.synth_state_dict(d, 0)
    lines = [f"score_bench {datetime.date.today().isoformat()} on {torch.cuda.get_device_name(0)}; config.yml dims, 3x224x672, L = {L}; "
             f"median of {REPS} alternating calls after {WARM} warm-up calls each, device events; decoder pass only (encoder output given)",
             f"{'dtype':5} {'images':>6} | {'fused ms':>9} {'(min-max)':>15} {'peak MB':>8} | {'logits ms':>9} {'(min-max)':>15} {'peak MB':>8} | "
             f"{'fused/logits':>12} {'max |dlogp|':>11}"]
    for dtype in ("bf16", "fp32"):
        for B in (64, 256):
            m = model_from_dims(d, dtype=dtype, max_batch=B, max_tokens=589)
            m.load_state_dict(sd)
            gen = torch.Generator(device="cuda").manual_seed(B)
            img = torch.rand((B, 3, 224, 672), generator=gen, device="cuda")
            trg = torch.randint(0, d.vocab - 3, (B, L), generator=gen, device="cuda")
            trg[:, 0] = d.bos
            enc = m.encoder(img)

            def fused():
                return m.decoder.score(trg, enc=enc).logp

            def logits_route():
                lg = m.decoder.net(trg[:, :-1].contiguous(), enc=enc)
                return torch.log_softmax(lg, -1).gather(-1, trg[:, 1:, None])[..., 0]

            for _ in range(WARM):
                fused(), logits_route()
            tf, tl, mf, ml, diff = [], [], 0, 0, 0.0
            for _ in range(REPS):
                a_ms, a_mem, a = timed(fused)
                b_ms, b_mem, b = timed(logits_route)
                tf.append(a_ms), tl.append(b_ms)
                mf, ml, diff = max(mf, a_mem), max(ml, b_mem), max(diff, float((a - b).abs().max()))
                del a, b
            f, l_ = statistics.median(tf), statistics.median(tl)
            lines.append(f"{dtype:5} {B:6d} | {f:9.2f} {f'({min(tf):.2f}-{max(tf):.2f})':>15} {mf / 2**20:8.1f} | {l_:9.2f} "
                         f"{f'({min(tl):.2f}-{max(tl):.2f})':>15} {ml / 2**20:8.1f} | {f / l_:12.3f} {diff:11.2e}")
            print(lines[-1], flush=True)
            del m, enc, img
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
