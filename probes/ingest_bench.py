"""What the image front end costs, by either ingest (profiles/ingest_cost.txt).

256 synthetic PIL images, uniform over the admissible sizes of the 224x672 canvas as in probes/ragged_bench.py, alternating modes L and
RGB (white background, dark strokes), the benchmark's model in bf16.  Both ways run alternating in ONE process on one build; median of
--reps repetitions after a warm-up of every route:
  (1) wall time from the image list to a container on the device (synchronised), ingest='host': preprocess_image per image, one .cuda() per
      image, pack_ragged -- the path that has always been there;
  (2) the same by ingest='device': OCRModel.ingest = one copy of the pixel bytes and one launch;
  (3) the ingest kernel's own time (events bound to the dispatch, txo_profile_read kind 4) beside the bytes it reads and writes;
  (4) TeXOCRWrapper.batch images/s end to end, both ways, greedy.

    python probes/ingest_bench.py [--images 256] [--reps 7] [--max-len 256] [--out profiles/ingest_cost.txt]"""
import argparse
import json
import os
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


def synthetic_images(n, seed):
    from PIL import Image
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n):
        h, w = int(rng.randint(1, 15)) * 16 - int(rng.randint(0, 16)), int(rng.randint(1, 43)) * 16 - int(rng.randint(0, 16))
        a = np.full((h, w) if k % 2 == 0 else (h, w, 3), 255, dtype=np.uint8)
        ys, xs = rng.randint(0, h, h * w // 8), rng.randint(0, w, h * w // 8)
        a[ys, xs] = rng.randint(0, 160, (len(ys),) + a.shape[2:])
        out.append(Image.fromarray(a))
    return out


def timed(f, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-len", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("ingest_bench: no GPU visible; nothing is measured without one")
    tmp = tempfile.mkdtemp()
    v = json.load(open(os.path.join(ROOT, "tests", "golden", "tokenizer_vocab_1k.json")))
    RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"]).save(os.path.join(tmp, "vocab.txt"))
    cfg = default_config(img_size=[224, 672])
    cfg["tokenizer_path"] = os.path.join(tmp, "vocab.txt")
    w = TeXOCRWrapper(cfg, dtype="bf16", max_batch=a.images)
    w.model.load_state_dict(synth.synth_state_dict(w.dims, 0))
    eng = w.model._engine
    imgs = synthetic_images(a.images, a.seed)

    def host_container():
        return ops.pack_ragged(w._images(imgs, "host"))

    def device_container():
        return w.model.ingest(imgs)

    routes = {
        "(1) list -> container, ingest='host'": host_container,
        "(2) list -> container, ingest='device'": device_container,
        "(4) batch() end to end, ingest='host'": lambda: w.batch(imgs, max_len=a.max_len, decode="greedy", ingest="host"),
        "(4) batch() end to end, ingest='device'": lambda: w.batch(imgs, max_len=a.max_len, decode="greedy", ingest="device"),
    }
    assert torch.equal(host_container()[0], device_container().box), "the two containers differ"
    assert routes["(4) batch() end to end, ingest='host'"]() == routes["(4) batch() end to end, ingest='device'"](), "the two results differ"
    for f in routes.values():                                      # warm-up of every route (the checks above were the first)
        f()
    times = {k: [] for k in routes}
    for _ in range(a.reps):                                        # alternating: one repetition of every route per round
        for k, f in routes.items():
            times[k] += timed(f, 1)
    eng.profile(1)                                                 # the kernel alone, in a pass of its own
    for _ in range(a.reps):
        p = device_container()
    torch.cuda.synchronize()
    k_ms, k_n = eng.profile_read(4)
    eng.profile(0)
    arrs = [np.asarray(im) for im in imgs]
    b_in, b_out = sum(x.size for x in arrs), p.box.numel() * 4
    b_host = sum(4 * w.dims.in_channels * int(h) * int(wd) for h, wd in p.sizes.tolist())

    lines = [f"ingest cost: {a.images} PIL images (L and RGB alternating), sizes uniform over the 224x672 canvas's, box {tuple(p.box.shape)}; "
             f"{torch.cuda.get_device_name(0)}; bf16, greedy, max_len {a.max_len}; median of {a.reps} alternating repetitions after warm-up",
             f"{'route':44s} {'ms':>10s} {'images/s':>10s}"]
    for k, ts in times.items():
        med = statistics.median(ts)
        lines.append(f"{k:44s} {med * 1e3:10.2f} {a.images / med:10.1f}   (min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f})")
    lines.append(f"(3) ingest_u8_kernel alone: {k_ms * 1e3:.1f} us mean of {k_n} launches (events bound to the dispatch); reads {b_in / 1e6:.2f} MB of pixels, "
                 f"writes {b_out / 1e6:.2f} MB: {(b_in + b_out) / (k_ms * 1e-3) / 1e12 if k_ms else 0:.2f} TB/s; the host path copies {b_host / 1e6:.2f} MB "
                 f"of float32 to the device in {a.images} copies, the device path {b_in / 1e6:.2f} MB of bytes in one")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
