#!/usr/bin/env python3
"""What the attention maps cost on top of the multi-position decoder forward (profiles/attn_maps_cost.txt).

config.yml dims on 224x672 images (N = 589), L = 257 (256 fed positions), 64 and 256 images, bf16 and fp32.  Per configuration the
calls alternate inside one process and the median of 7 rounds is reported:
  decode_prefill (no logits)                     the pass without maps (the parent's path)
  decode_attn, head mean only                    what OCRModel.align runs
  decode_attn, self + cross + head mean          everything (the per-head tensors are allocated once, outside the timing)
  model.score(src, trg) / model.align(src, trg)  the two facades end to end, encoder included

Usage:  python probes/attn_bench.py [--batches 64 256] [--dtypes bf16 fp32] [--out profiles/attn_maps_cost.txt]
"""
import argparse
import datetime
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from texocr_amd import _lib, synth                                      # noqa: E402
from texocr_amd.config import Dims                                      # noqa: E402
from texocr_amd.model import model_from_dims                            # noqa: E402

ROUNDS = 7


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def run(dtype, B, lines):
    d = Dims(canvas=672)
    m = model_from_dims(d, dtype=dtype, max_batch=B)
    m.load_state_dict(synth.synth_state_dict(d, 0))
    eng = m._engine
    img = torch.from_numpy(synth.synth_images(B, 3, 224, 672, seed=1)).cuda()
    g = torch.Generator().manual_seed(2)
    trg = torch.randint(0, d.vocab - 3, (B, d.max_len + 1), generator=g).cuda()
    trg[:, 0] = d.bos
    x = trg[:, :-1].contiguous()
    t, N, Ld, heads = x.shape[1], d.n_tokens(224, 672), d.dec_layers, d.dec_heads
    eng.decode_begin(m.encoder(img))
    mean = torch.empty((Ld, B, t, N), device="cuda")
    per_head = (Ld * B * heads * t * (t + N)) * 4
    full = per_head < 40e9                                               # (1.8 GB at 64 images, 7.1 GB at 256)
    sp = torch.empty((Ld, B, heads, t, t), device="cuda") if full else None
    cp = torch.empty((Ld, B, heads, t, N), device="cuda") if full else None
    stream = torch.cuda.current_stream().cuda_stream

    def attn(s_, c_, m_):
        _lib.check(eng.lib.txo_decode_attn(eng.handle, x.data_ptr(), t, None, s_.data_ptr() if s_ is not None else None,
                                          c_.data_ptr() if c_ is not None else None, m_.data_ptr() if m_ is not None else None, stream))

    calls = {"decode_prefill": lambda: eng.decode_prefill(x, want_logits=False),
             "decode_attn head mean": lambda: attn(None, None, mean)}
    if full:
        calls["decode_attn self+cross+mean"] = lambda: attn(sp, cp, mean)
    calls["model.score"] = lambda: m.score(img, trg)
    calls["model.align"] = lambda: m.align(img, trg)
    for fn in calls.values():                                            # warm-up
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, fn in calls.items():
            ms[k].append(timed(fn))
    base = statistics.median(ms["decode_prefill"])
    for k in calls:
        med = statistics.median(ms[k])
        ref = statistics.median(ms["model.score"]) if k == "model.align" else base
        rel = "" if k in ("decode_prefill", "model.score") else f"  ({(med / ref - 1) * 100:+.1f} % against {'model.score' if k == 'model.align' else 'decode_prefill'})"
        lines.append(f"{dtype:5s} B={B:<4d} {k:30s} {med:9.2f} ms   min {min(ms[k]):9.2f}  max {max(ms[k]):9.2f}{rel}")
        print(lines[-1], flush=True)
    if not full:
        lines.append(f"{dtype:5s} B={B:<4d} per-head tensors not made: {per_head / 1e9:.0f} GB")
        print(lines[-1], flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--dtypes", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_maps_cost.txt"))
    a = ap.parse_args()
    lines = [f"# probes/attn_bench.py: config.yml dims, 224x672 (N = 589), 256 fed positions, median of {ROUNDS} alternating rounds, "
             f"{torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}"]
    for dtype in a.dtypes:
        for B in a.batches:
            run(dtype, B, lines)
            torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
