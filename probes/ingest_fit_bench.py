"""What fitting oversized images to the canvas costs, by either ingest (profiles/ingest_fit_cost.txt).

256 synthetic PIL images for the 224x672 canvas, modes L and RGB alternating (white background, dark strokes): every even one lies within
the canvas (sizes as in probes/ingest_bench.py), every odd one is 1.5-4 times over it on both sides.  The benchmark's model in bf16.  Both
ways run alternating in ONE process on one build; median of --reps repetitions after a warm-up of every route:
  (1) wall time from the image list to a container on the device (synchronised), ingest='host', fit='canvas': PIL's resize of the oversized
      images, then preprocess_image per image, one .cuda() per image, pack_ragged;
  (2) the same by ingest='device': OCRModel.ingest(fit=True) = one copy of the RAW pixel bytes and the two launches of txo_ingest_u8_fit;
  (3) the new kernels alone (events bound to the dispatches, txo_profile_read kind 4) beside the bytes they read and write.
No ratio is fixed in advance: both numbers and the machine are recorded.

    python probes/ingest_fit_bench.py [--images 256] [--reps 7] [--out profiles/ingest_fit_cost.txt]"""
import argparse
import json
import os
import platform
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from texocr_amd import ops, synth
from texocr_amd.config import default_config
from texocr_amd.tokenizer import RegExTokenizer
from texocr_amd.wrapper import TeXOCRWrapper


def synthetic_images(n, seed, canvas=(224, 672)):
    from PIL import Image
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n):
        h, w = int(rng.randint(1, 15)) * 16 - int(rng.randint(0, 16)), int(rng.randint(1, 43)) * 16 - int(rng.randint(0, 16))
        if k % 2:                                                  # 1.5 - 4 times over the canvas, on both sides
            s = 1.5 + 2.5 * rng.rand()
            h, w = int(canvas[0] * s) + int(rng.randint(0, 16)), int(canvas[1] * s) + int(rng.randint(0, 16))
        a = np.full((h, w) if k % 4 < 2 else (h, w, 3), 255, dtype=np.uint8)
        ys, xs = rng.randint(0, h, h * w // 8), rng.randint(0, w, h * w // 8)
        a[ys, xs] = rng.randint(0, 160, (len(ys),) + a.shape[2:])
        out.append(Image.fromarray(a))
    return out


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("ingest_fit_bench: no GPU visible; nothing is measured without one")
    import PIL
    tmp = tempfile.mkdtemp()
    v = json.load(open(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab_1k.json")))
    RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"]).save(os.path.join(tmp, "vocab.txt"))
    cfg = default_config(img_size=[224, 672])
    cfg["tokenizer_path"] = os.path.join(tmp, "vocab.txt")
    w = TeXOCRWrapper(cfg, dtype="bf16", max_batch=a.images)
    w.model.load_state_dict(synth.synth_state_dict(w.dims, 0))
    eng = w.model._engine
    imgs = synthetic_images(a.images, a.seed)
    Fh, Fw = w.dims.canvas_hw
    n_over = sum(ops.fit_size(im.size[1], im.size[0], Fh, Fw) != (im.size[1], im.size[0]) for im in imgs)

    def host_container():
        return ops.pack_ragged(w._images(imgs, "host", "canvas"))

    def device_container():
        return w.model.ingest(imgs, fit=True)

    routes = {"(1) list -> container, ingest='host', fit='canvas'": host_container, "(2) list -> container, ingest='device', fit='canvas'": device_container}
    assert torch.equal(host_container()[0], device_container().box), "the two containers differ"
    for f in routes.values():                                      # warm-up of every route (the check above was the first)
        f()
    times = {k: [] for k in routes}
    for _ in range(a.reps):                                        # alternating: one repetition of every route per round
        for k, f in routes.items():
            times[k].append(timed(f))
    t_pil = []
    for _ in range(a.reps):                                        # the PIL share of (1): the resizes alone
        t0 = time.perf_counter()
        for im in imgs:
            w._fitted(im)
        t_pil.append(time.perf_counter() - t0)
    eng.profile(1)                                                 # the kernels alone, in a pass of their own
    for _ in range(a.reps):
        p = device_container()
    torch.cuda.synchronize()
    k_ms, k_n = eng.profile_read(4)
    eng.profile(0)
    call_ms = k_ms * k_n / a.reps                                   # both launches of one call
    arrs = [np.asarray(im) for im in imgs]
    b_in, b_out = sum(x.size for x in arrs), p.box.numel() * 4
    b_mid = 0
    for x in arrs:
        fh, fw = ops.fit_size(x.shape[0], x.shape[1], Fh, Fw)
        if fw != x.shape[1]:
            b_mid += x.shape[0] * fw * (1 if x.ndim == 2 else 3)
    moved = b_in + 2 * b_mid + b_out                               # the intermediate is written once and read once

    lines = [f"fit-to-canvas ingest cost: {a.images} PIL images (L and RGB), {a.images - n_over} within the {Fh}x{Fw} canvas, {n_over} 1.5-4x over it; box "
             f"{tuple(p.box.shape)}; {torch.cuda.get_device_name(0)}; host {platform.processor() or platform.machine()}, {os.cpu_count()} CPUs, "
             f"PIL {PIL.__version__}, torch {torch.__version__}; median of {a.reps} alternating repetitions after warm-up",
             f"{'route':56s} {'ms':>10s} {'images/s':>10s}"]
    for k, ts in times.items():
        med = statistics.median(ts)
        lines.append(f"{k:56s} {med * 1e3:10.2f} {a.images / med:10.1f}   (min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f})")
    lines.append(f"    of (1), PIL's resize of the {n_over} oversized images alone: {statistics.median(t_pil) * 1e3:.2f} ms "
                 f"(min {min(t_pil) * 1e3:.2f}, max {max(t_pil) * 1e3:.2f})")
    lines.append(f"(3) fit_rows_kernel + ingest_fit_kernel alone: {call_ms * 1e3:.1f} us per call ({k_n} launches in {a.reps} calls, events bound to the "
                 f"dispatch); reads {b_in / 1e6:.2f} MB of pixels, writes and re-reads {b_mid / 1e6:.2f} MB of intermediates, writes {b_out / 1e6:.2f} MB: "
                 f"{moved / (call_ms * 1e-3) / 1e12 if call_ms else 0:.2f} TB/s")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
