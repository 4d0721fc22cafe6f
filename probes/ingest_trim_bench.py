"""What trimming images to their ink costs and saves, by either ingest (profiles/ingest_trim_cost.txt).

256 synthetic PIL images for the 224x672 canvas, modes L and RGB alternating: a white frame (sizes as in probes/ingest_bench.py) with dark
strokes inside an ink box whose AREA is a quarter to a half of the frame, placed at random.  The benchmark's model in bf16.  All routes run
alternating in ONE process on one build; median of --reps repetitions after a warm-up of every route:
  (1) wall time from the image list to a container on the device (synchronised), ingest='host', trim='ink': ops.trim_view (numpy) and PIL's
      crop per image, then preprocess_image per image, one .cuda() per image, pack_ragged;
  (2) the same by ingest='device': OCRModel.ingest(trim=) = one copy of the RAW pixel bytes, the ink search (one launch, one wait) and one
      launch of the pitched ingest kernel;
  (3) trim_bbox_kernel alone and the pitched ingest kernel alone (events bound to the dispatches, txo_profile_read kind 4, a pass each)
      beside the bytes they read and write;
  (4) wrapper.batch end to end (greedy), with and without trim, by either ingest, on the same images.
No ratio is fixed in advance: every number and the machine are recorded.

    python probes/ingest_trim_bench.py [--images 256] [--reps 7] [--out profiles/ingest_trim_cost.txt]"""
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


def synthetic_images(n, seed):
    from PIL import Image
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n):
        h, w = int(rng.randint(2, 15)) * 16 - int(rng.randint(0, 16)), int(rng.randint(4, 43)) * 16 - int(rng.randint(0, 16))
        side = np.sqrt(0.25 + 0.25 * rng.rand())                  # the ink box's share of either side: its area is 1/4 .. 1/2 of the frame
        bh, bw = max(1, int(h * side)), max(1, int(w * side))
        y0, x0 = int(rng.randint(0, h - bh + 1)), int(rng.randint(0, w - bw + 1))
        a = np.full((h, w) if k % 2 == 0 else (h, w, 3), 255, dtype=np.uint8)
        ys, xs = y0 + rng.randint(0, bh, bh * bw // 8 + 2), x0 + rng.randint(0, bw, bh * bw // 8 + 2)
        ys[:2], xs[:2] = (y0, y0 + bh - 1), (x0, x0 + bw - 1)     # the box's corners are ink
        a[ys, xs] = rng.randint(0, 120, (len(ys),) + a.shape[2:])
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
    ap.add_argument("--max-len", type=int, default=256)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("ingest_trim_bench: no GPU visible; nothing is measured without one")
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
    rule = (ops.TRIM_LEVEL, ops.TRIM_MARGIN)
    dev = torch.device("cuda", eng.device)

    routes = {
        "(1) list -> container, ingest='host', trim='ink'": lambda: ops.pack_ragged(w._images(imgs, "host", "none", rule)),
        "(2) list -> container, ingest='device', trim='ink'": lambda: w.model.ingest(imgs, trim=rule),
        "    list -> container, ingest='host', untrimmed": lambda: ops.pack_ragged(w._images(imgs, "host")),
        "    list -> container, ingest='device', untrimmed": lambda: w.model.ingest(imgs),
        "(4) batch() end to end, ingest='host', trim='ink'": lambda: w.batch(imgs, max_len=a.max_len, decode="greedy", ingest="host", trim="ink"),
        "(4) batch() end to end, ingest='device', trim='ink'": lambda: w.batch(imgs, max_len=a.max_len, decode="greedy", ingest="device", trim="ink"),
        "(4) batch() end to end, ingest='host', untrimmed": lambda: w.batch(imgs, max_len=a.max_len, decode="greedy", ingest="host"),
        "(4) batch() end to end, ingest='device', untrimmed": lambda: w.batch(imgs, max_len=a.max_len, decode="greedy", ingest="device"),
    }
    host, packed = routes["(1) list -> container, ingest='host', trim='ink'"](), routes["(2) list -> container, ingest='device', trim='ink'"]()
    assert torch.equal(host[0], packed.box) and torch.equal(host[1], packed.sizes), "the two containers differ"
    whole = w.model.ingest(imgs)
    for f in routes.values():                                      # warm-up of every route
        f()
    times = {k: [] for k in routes}
    for _ in range(a.reps):                                        # alternating: one repetition of every route per round
        for k, f in routes.items():
            times[k].append(timed(f))
    t_np = []
    for _ in range(a.reps):                                        # the numpy + PIL share of (1): the views and the crops alone
        t0 = time.perf_counter()
        for im in imgs:
            w._trimmed(im, rule)
        t_np.append(time.perf_counter() - t0)
    # the kernels alone, a pass each
    staged, devs, src, shapes = ops.plan_u8(imgs)
    bufs = [staged.to(dev)] + devs
    views = packed.views
    Hc, Wc = ops.box_u8(ops.view_shapes(shapes, views))
    eng.profile(1)
    for _ in range(a.reps):
        torch.ops.texocr.ingest_trim_views(bufs, src, shapes, eng.id, *rule)
    torch.cuda.synchronize()
    bbox_ms, bbox_n = eng.profile_read(4)
    eng.profile(0)
    eng.profile(1)
    for _ in range(a.reps):
        torch.ops.texocr.ingest_u8_view(bufs, src, shapes, views, eng.id, w.dims.in_channels, 0, 0, Hc, Wc)
    torch.cuda.synchronize()
    view_ms, view_n = eng.profile_read(4)
    eng.profile(0)
    b_in = int(shapes.to(torch.int64).prod(dim=1).sum())
    b_view = int((views[:, 2].to(torch.int64) * views[:, 3] * shapes[:, 2]).sum())
    b_out = packed.box.numel() * 4

    def patches(sizes):
        return int((sizes[:, 0].to(torch.int64) // 16 * (sizes[:, 1] // 16)).sum())
    lines = [f"trim-to-ink ingest cost: {a.images} PIL images (L and RGB alternating), ink box 1/4 - 1/2 of the frame's area, level {rule[0]}, margin {rule[1]}; "
             f"box {tuple(whole.box.shape)} untrimmed -> {tuple(packed.box.shape)} trimmed, {patches(whole.sizes)} -> {patches(packed.sizes)} patches in all; "
             f"{torch.cuda.get_device_name(0)}; host {platform.processor() or platform.machine()}, {os.cpu_count()} CPUs, PIL {PIL.__version__}, "
             f"torch {torch.__version__}; bf16, greedy, max_len {a.max_len}; median of {a.reps} alternating repetitions after warm-up",
             f"{'route':56s} {'ms':>10s} {'images/s':>10s}"]
    for k, ts in times.items():
        med = statistics.median(ts)
        lines.append(f"{k:56s} {med * 1e3:10.2f} {a.images / med:10.1f}   (min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f})")
    lines.append(f"    of (1), ops.trim_view + PIL's crop of the {a.images} images alone: {statistics.median(t_np) * 1e3:.2f} ms "
                 f"(min {min(t_np) * 1e3:.2f}, max {max(t_np) * 1e3:.2f})")
    lines.append(f"(3) trim_bbox_kernel alone: {bbox_ms * 1e3:.1f} us mean of {bbox_n} launches (events bound to the dispatch); reads {b_in / 1e6:.2f} MB of "
                 f"pixels, writes 16 bytes per image: {b_in / (bbox_ms * 1e-3) / 1e12 if bbox_ms else 0:.3f} TB/s")
    lines.append(f"(3) ingest_u8_kernel<pitched> alone: {view_ms * 1e3:.1f} us mean of {view_n} launches; reads {b_view / 1e6:.2f} MB of the views' pixels, "
                 f"writes {b_out / 1e6:.2f} MB: {(b_view + b_out) / (view_ms * 1e-3) / 1e12 if view_ms else 0:.2f} TB/s")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
