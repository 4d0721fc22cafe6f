#!/usr/bin/env python3
"""Headline benchmark: images/sec of OCRModel.generate() on synthetic 3x224x672 batches, greedy,
max_len=256 (BASELINE.json configs[1]: config.yml dims, batch 64 per GPU, bf16 as that config names).

A "step" is one generate() call over one batch: ViT patch-embed + encoder stack, cross-K/V projection,
256 KV-cached decode steps, and (under torch.distributed) the RCCL all-gather of the token ids.  Inputs are
resident in HBM before the timed region.  One process per GPU (the driver launches torch.distributed.run for
N>1); rank 0 prints ONE JSON line.

Objects on the line besides the contract's fields:
  roofline     -- decode-step cross-attention kernel (the HBM-bound kernel north_star names): algorithmic
                  bytes per launch = B*heads*2*N*64*sizeof(dtype), divided by the kernel's average launch
                  duration measured with HIP events bound to the dispatches of the LAST timed step.
                  `traffic` = HBM bytes per launch from the PMC counters, measured in this run by rocprofv3 --pmc child passes of this
                  script (live_pmc; N=1 default run) or, failing that, from the tracked profiles/ file -- `traffic_source` says which.
  cpu_baseline -- the oracle (oracle/cpu_ref.py, "port") on this host: `value` = recompute mode = the reference's
                  algorithm (no KV cache, decoder.py:97-103) on a bounded sample; `cached` = the same oracle with a KV cache.
  fp32_parity_mode, sampled_decode, b256, cfg4, cfg5_beam, row_stop_b256, hybrid_default (N=1 only, after the timed region; --no-extras skips them):
                  the token-exact fp32 engine on the same workload; the reference's default (sampled) decode; batch 256 (the north-star HBM target: cross-attention
                  >= 50 % of 8 TB/s); BASELINE configs[3] (ViT-Base 12L/768d + 6L decoder, B=256: encoder >= 40 % of the
                  bf16 MFMA peak).
These objects (and the live PMC child passes behind `traffic`) are measured with --full only.  A plain run sets up, settles and warms
up, times --steps steps and prints the contract's fields; --dump-outputs DIR also writes the tokens of the last timed step as
DIR/tokens.npy (float32), so that two builds can be compared output for output on identical inputs.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle-seconds", type=float, default=1.5,
                    help="untimed: repeat the step for this long before the W warmup steps so that a freshly started GPU "
                         "reaches its steady clocks (the first process on a fresh box measured 8 %% slower without it)")
    ap.add_argument("--batch", type=int, default=64, help="images per GPU per step")
    ap.add_argument("--height", type=int, default=224)
    ap.add_argument("--width", type=int, default=672)
    ap.add_argument("--max-len", type=int, default=256)
    ap.add_argument("--dtype", default=os.environ.get("TEXOCR_BENCH_DTYPE", "bf16"), choices=["bf16", "fp32"])
    ap.add_argument("--full", action="store_true",
                    help="also measure everything besides the headline figure: live PMC passes, roofline, the side measurements and the "
                         "CPU baseline (the --no-* options below switch parts of it off)")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps write the tokens of the last one as DIR/tokens.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline-full", action="store_true",
                    help="with --full: also run the WHOLE un-sampled reference-algorithm generate on the CPU (minutes): validates the sampled estimate")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the fp32 / batch-256 / config-4 side measurements")
    ap.add_argument("--no-live-pmc", action="store_true",
                    help="do not collect the HBM counters of the dominant launches in this run (rocprofv3 --pmc child passes, N=1 only); "
                         "`traffic` then comes from the tracked profiles/ file and says so")
    ap.add_argument("--model", default="default", choices=["default", "cfg4"],
                    help="cfg4 = BASELINE configs[3] (ViT-Base 12L/768d encoder + 6L/768d decoder) as the main workload: for profiling "
                         "runs; the headline metric is quoted on the default model")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if not a.full:                                        # a plain run measures the headline figure only
        a.no_cpu_baseline = a.no_roofline = a.no_extras = a.no_live_pmc = True
    return a


def dump_outputs(dirname, arrays, limit=64 << 20):
    """Writes each array as dirname/<name>.npy in float32.  Beyond `limit` bytes in all, every array keeps a fixed, seeded sample
    of its rows (the same rows from run to run)."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    arrays = {k: np.asarray(v, dtype=np.float32) for k, v in arrays.items()}
    total = sum(v.nbytes for v in arrays.values())
    for name, v in arrays.items():
        if total > limit:
            keep = max(1, int(v.shape[0] * limit // total))
            v = v[np.sort(np.random.Generator(np.random.PCG64(0)).choice(v.shape[0], keep, replace=False))]
        np.save(os.path.join(dirname, f"{name}.npy"), v)


LIVE_PMC = {}          # kind -> HBM bytes per launch measured in THIS run (live_pmc), read where the roofline objects are built


def live_pmc(a):
    """HBM bytes per launch of the dominant kernels from the PMC counters, collected in THIS run the way MI355X_MICROARCH.md's HBM section
    prescribes: one counter per rocprofv3 pass (FETCH_SIZE, WRITE_SIZE), --kernel-trace only, read bytes = 2 * FETCH_SIZE (gfx950 counts
    16-byte-per-lane streams at half) + WRITE_SIZE.  Each pass is a CHILD run of this script (one generate, no side measurements) started
    BEFORE this process touches the GPU.  Kinds: 'persist' = the persistent decode launch of the headline workload (all max_len
    positions); 'b256' = the whole-batch cross-attention launch at batch 256 (one row range, 24 positions: bytes per launch do not
    depend on the position).  Anything that goes wrong leaves the kind out: the line then quotes the tracked profiles/ file and says so."""
    import csv, glob, shutil, subprocess, tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return
    tmp = tempfile.mkdtemp(prefix="txo_pmc_", dir="/tmp")
    base = [sys.executable, os.path.abspath(__file__), "--steps", "1", "--warmup", "0", "--settle-seconds", "0", "--dtype", a.dtype,
            "--height", str(a.height), "--width", str(a.width), "--no-cpu-baseline", "--no-roofline", "--no-extras", "--no-live-pmc"]
    kinds = [("persist", {"TXO_PERSIST": "1"}, ["--batch", str(a.batch), "--max-len", str(a.max_len)], "decode_persist_kernel")]
    if not a.no_extras and a.dtype == "bf16":
        kinds.append(("b256", {"TXO_PERSIST": "0", "TXO_LANES": "1"}, ["--batch", "256", "--max-len", "24"], "lat_core_kernel"))
    t_start = time.perf_counter()
    try:
        for kind, env_extra, args, kname in kinds:
            vals = {}
            for counter in ("FETCH_SIZE", "WRITE_SIZE"):
                if time.perf_counter() - t_start > 240:                 # bounded: the default run has to finish within minutes
                    raise TimeoutError
                d = os.path.join(tmp, kind, counter)
                env = dict(os.environ, TMPDIR="/tmp", **env_extra)
                # own session: a timeout must end the profiler AND the python child it started (a survivor would decode beside the timed region)
                pr = subprocess.Popen([exe, "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", d, "--"] + base + args,
                                      env=env, cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
                try:
                    pr.wait(timeout=240)
                except subprocess.TimeoutExpired:
                    import signal
                    try:
                        os.killpg(pr.pid, signal.SIGKILL)
                    except OSError:
                        pass
                    pr.wait()
                    raise
                got = []
                for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
                    for r in csv.DictReader(open(f)):
                        if r.get("Counter_Name") == counter and kname in r.get("Kernel_Name", ""):
                            got.append(float(r["Counter_Value"]))
                if not got:
                    raise RuntimeError(f"no {counter} rows for {kname}")
                vals[counter] = sum(got) / len(got)                     # KB per launch
            LIVE_PMC[kind] = {"traffic_bytes": int(2 * vals["FETCH_SIZE"] * 1024 + vals["WRITE_SIZE"] * 1024),
                              "source": "measured in this run: two rocprofv3 --pmc child passes of this script (FETCH_SIZE, WRITE_SIZE; "
                                        "--kernel-trace only), read bytes = 2 x FETCH_SIZE (gfx950) + WRITE_SIZE, average over the pass's launches"}
    except Exception as e:                                  # the line then quotes the tracked profiles/ file -- and says why
        LIVE_PMC["error"] = f"{type(e).__name__}: {e}"[:200]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(dims, sd_np, a):
    """The reference algorithm on the host CPU through the oracle (oracle/cpu_ref.py), on the SAME workload (64 images,
    256 greedy steps), bounded to tens of seconds by sampling:

    * recompute mode = what the reference does (decoder.py:97-103): every step pushes the WHOLE prefix through the decoder
      and re-projects the cross-attention K/V.  A step's cost depends on the prefix length only, so the step is timed at nine
      prefix lengths 1..256 with the real batch (random valid tokens as the prefix) and the 256 step times are interpolated
      linearly between them; the encoder is timed once.  value = images / (encoder + sum of step times).
    * cached mode = the oracle's KV-cached form, run in full on 16 images.
    torch's intra-op thread count is picked by a short probe (on the 2-socket GPU host 128 threads run this workload several
    times SLOWER than 32)."""
    import numpy as np
    import torch
    from oracle import cpu_ref
    from texocr_amd import synth
    sd = cpu_ref.to_torch_sd(sd_np)
    B, T = a.batch, a.max_len
    img = torch.from_numpy(synth.synth_images(B, dims.in_channels, a.height, a.width, seed=1234))
    rng = np.random.Generator(np.random.PCG64(7))

    def prefix(n, t):
        x = torch.from_numpy(rng.integers(0, dims.vocab - 3, size=(n, t), dtype=np.int64))
        x[:, 0] = dims.bos
        return x
    with torch.no_grad():
        # thread count: fastest of a few candidates on the REAL step -- the benchmark's own batch at a mid prefix length (a small
        # probe picked 64 threads on the 2-socket GPU host, where 16 run this step 1.5x faster)
        ncpu = os.cpu_count() or 1
        encB = torch.zeros((B, dims.n_tokens(a.height, a.width), dims.embed_dim))
        xp = prefix(B, min(T, 64))
        best_nt, best_dt, probe = torch.get_num_threads(), None, {}
        for nt in sorted({n for n in (8, 16, 32, 64) if 1 <= n <= ncpu} | ({ncpu} if ncpu < 8 else set())):
            torch.set_num_threads(nt)
            t0 = time.perf_counter()
            cpu_ref.decoder_net(sd, xp, encB)
            dt = time.perf_counter() - t0
            probe[nt] = round(dt, 3)
            if best_dt is None or dt < best_dt:
                best_nt, best_dt = nt, dt
            if dt > 1.5 * best_dt:                    # past the optimum (more threads only get slower on the 2-socket host: 128 -> 2.1 s,
                break                                 # 256 -> 30 s for a step that takes 0.6 s with 16): do not spend the budget there
        torch.set_num_threads(best_nt)
        t0 = time.perf_counter()
        enc = cpu_ref.encode(sd, img)
        t_enc = time.perf_counter() - t0
        ts = sorted({min(T, x) for x in (1, 32, 64, 96, 128, 160, 192, 224, T)})
        cost = []
        for t in ts:
            x = prefix(B, t)
            runs = []
            for _ in range(2):
                t0 = time.perf_counter()
                cpu_ref.decoder_net(sd, x, enc)[:, -1, :].argmax(-1)              # decoder.py:103-108, greedy
                runs.append(time.perf_counter() - t0)
            # the MEAN of the two runs: the minimum under-estimated the real loop by 14 % (profiles/r03_cpu_baseline_full.json: the whole
            # un-sampled batch took 246.8 s on this host class where min-based sampling predicted 213 s)
            cost.append(sum(runs) / len(runs))
        steps = np.interp(np.arange(1, T + 1), ts, cost)
        total = t_enc + float(steps.sum())
        measured = t_enc + 2 * sum(cost)                                      # two runs per sampled prefix length
        bc = min(16, B)
        t0 = time.perf_counter()
        tc = cpu_ref.generate_cached(sd, img[:bc], dims.bos, dims.eos, T, enc=enc[:bc])
        dtc = time.perf_counter() - t0
        assert tc.shape[1] == T
        full = None
        if a.cpu_baseline_full:                       # one-off validation of the interpolation: the whole batch, every step, no sampling
            t0 = time.perf_counter()
            tr = cpu_ref.generate_recompute(sd, img, dims.bos, dims.eos, T)
            dtf = time.perf_counter() - t0
            assert tr.shape == (B, T)
            full = {"value": round(B / dtf, 4), "unit": "images/sec", "seconds": round(dtf, 1),
                    "sample": f"the WHOLE batch, all {T} steps, un-sampled (oracle recompute mode), {best_nt} threads"}
    out = {"value": round(B / total, 4), "unit": "images/sec", "cores": int(best_nt), "kind": "port",
            "sample": f"oracle recompute mode (reference algorithm, no KV cache) on the benchmark's own batch: {B} images "
                      f"{dims.in_channels}x{a.height}x{a.width}; encoder timed once ({t_enc:.1f} s), the full-prefix step timed at prefix "
                      f"lengths {ts} ({', '.join(f'{c:.2f}' for c in cost)} s) and interpolated over the {T} steps: {measured:.1f} s of CPU "
                      f"work measured, {total:.0f} s estimated for the whole batch; torch CPU fp32, {best_nt} threads (fastest on the real "
                      f"{B}-image step at prefix length {xp.shape[1]}: seconds by thread count {probe}) on {ncpu} logical CPUs; "
                      f"THIS host's estimate (the figure is per host: driver boxes of rounds 3 and 4 gave 0.267 and 0.502 images/s); the "
                      f"interpolation was validated once, on a 2 x EPYC 9575F GPU box, against the whole un-sampled batch "
                      f"(profiles/r03_cpu_baseline_full.json: 246.8 s = 0.259 images/s where that box's sampled estimate was 0.26-0.27)",
            "host": {"logical_cpus": int(ncpu), "cpu_model": _cpu_model()},
            "cached": {"value": round(bc / dtc, 3), "unit": "images/sec",
                       "sample": f"oracle KV-cached mode, {bc} images, all {T} steps, {dtc:.1f} s wall"}}
    if full:
        out["full_run"] = full
    return out


def make_step(dist_on, generate_no_eos, generate_default, imgs, max_len, eos, bos, global_batch, expect_full=True):
    """One benchmark step = one pass of the hot path over one batch.

    Under torch.distributed (also with one rank) every rank decodes ITS images to max_len with the eos test off
    (generate_no_eos(images, max_len) -> (b, max_len) tokens), ONE all-gather of the token ids follows, and the reference's
    GLOBAL eos break (decoder.py:115-116) is applied to the gathered batch (texocr_amd/dist.py: sharded_generate).  Without
    a process group it is model.generate() itself.  tests/test_host_cpu.py runs this very function on two gloo ranks with the
    oracle as the per-rank generator."""
    from texocr_amd.dist import sharded_generate

    def step(i):
        if dist_on:
            toks = sharded_generate(generate_no_eos, imgs[i & 1], max_len, eos, bos=bos, images_are_local=True,
                                    global_batch=global_batch, force_collective=True)
        else:
            toks = generate_default(imgs[i & 1], max_len)                # eos never fires for every row with random weights
        if expect_full and toks.shape[1] != max_len:
            raise RuntimeError(f"expected {max_len} decode steps, got {toks.shape[1]}")
        return toks
    return step


def timed(model, img, max_len, warm, steps, **gen_kw):
    import torch
    for _ in range(warm):
        model.generate(img, max_len, **gen_kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = model.generate(img, max_len, **gen_kw)
    torch.cuda.synchronize()
    assert out.shape[1] == max_len
    return (time.perf_counter() - t0) / steps


def enc_flop(dims, B, N):
    """encoder (patch-embed + ViT stack) FLOPs, SURVEY 8d: 2(N-1)C*256*D + Le*(N(10DI + 6DF) + 4N^2 I) per image"""
    D_, I_, F_, Le = dims.embed_dim, dims.enc_inner, dims.enc_ffn, dims.enc_layers
    return B * (2 * (N - 1) * dims.in_channels * 256 * D_ + Le * (N * (10 * D_ * I_ + 6 * D_ * F_) + 4 * N * N * I_))


def beam_measurement(dtype, a, dev, B=128, k=5, widths=(224, 448, 672, 896)):
    """BASELINE configs[4] on one GPU: beam search k=5 (a build extension: the reference has none) over 128 images per
    width bucket, widths 224..896, max_len as the headline; images/s over the four buckets together."""
    import torch
    from texocr_amd import synth
    from texocr_amd.config import Dims
    from texocr_amd.model import model_from_dims
    d = Dims(canvas=max(widths))
    m = model_from_dims(d, dtype=dtype, max_batch=B * k, max_tokens=d.n_tokens(224, max(widths)))
    m.load_state_dict(synth.synth_state_dict(d, 0))
    m.eos_token = None                                    # every position runs
    g = torch.Generator(device=dev).manual_seed(977)
    per, tot = {}, 0.0
    for W in widths:
        img = torch.rand((B, d.in_channels, 224, W), generator=g, device=dev, dtype=torch.float32)
        m.generate(img, 16, beam=k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.generate(img, a.max_len, beam=k)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        per[f"224x{W}"] = round(B / dt, 1)
        tot += dt
    out = {"value": round(B * len(widths) / tot, 1), "unit": "images/sec", "beams": k, "images_per_bucket": B, "images_per_sec_by_width": per,
           "dtype": dtype, "max_len": a.max_len,
           "workload": "BASELINE configs[4] on ONE GPU: beam search k=5, 128 images per width bucket, widths 224..896 (bucketed by exact size)"}
    del m
    torch.cuda.empty_cache()
    return out


def backbone_flop(B, H, W):
    """ResNetV2 [2,4,6] backbone of the default factory (resnet.py:200-254) + the 1x1 projection, FLOPs (2 * MAC) for B images of 1 x H x W:
    stem 7x7/2 (1 -> 64), then per stage i (channels 256/512/1024 at strides 4/8/16) its bottlenecks: 1x1 cin->mid, 3x3 mid->mid, 1x1 mid->cout,
    and the first block's 1x1 downsample."""
    f = 0.0
    h, w = (H + 1) // 2, (W + 1) // 2
    f += 2.0 * h * w * 64 * 49
    h, w = (h + 1) // 2, (w + 1) // 2
    cin = 64
    for st, (depth, cout) in enumerate(zip((2, 4, 6), (256, 512, 1024))):
        mid = cout // 4
        for i in range(depth):
            stride = 2 if (i == 0 and st > 0) else 1
            ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
            if i == 0:
                f += 2.0 * ho * wo * cin * cout
            f += 2.0 * h * w * cin * mid + 2.0 * ho * wo * 9 * mid * mid + 2.0 * ho * wo * mid * cout
            h, w, cin = ho, wo, cout
    f += 2.0 * h * w * 1024 * 256
    return B * f


def hybrid_measurement(dtype, a, dev, B=64):
    """The model create_model(config/config.yml) actually builds: hybrid ResNetV2 [2,4,6] embedder on the full
    1 x 160 x 1008 canvas (631 tokens), config.yml dims behind it; greedy, max_len as the headline.  encoder_ms = backbone + ViT stack (wall time
    of back-to-back encodes); the backbone's share is that minus the ViT stack alone, measured on the plain-patch model at the same token count
    (vit_stack_ms)."""
    import torch
    from texocr_amd import synth
    from texocr_amd.config import Dims, reference_config
    from texocr_amd.model import model_from_dims
    d = Dims.from_config(reference_config())
    H, W = d.canvas_hw
    N = d.n_tokens(H, W)
    m = model_from_dims(d, dtype=dtype, max_batch=B, max_tokens=N)
    m.load_state_dict(synth.synth_state_dict(d, 0))
    g = torch.Generator(device=dev).manual_seed(99)
    img = torch.rand((B, 1, H, W), generator=g, device=dev, dtype=torch.float32)
    sec = timed(m, img, a.max_len, 2, 5)
    eng = m._engine

    def enc_ms(model, x, reps=5):
        for _ in range(2): model.encoder(x)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(reps): model.encoder(x)
        torch.cuda.synchronize()
        return 1000 * (time.perf_counter() - t0) / reps
    e_ms = enc_ms(m, img)
    persistent = eng.query(0) == 1
    del m
    torch.cuda.empty_cache()
    # the ViT stack alone at the same token count: plain-patch model on a 3 x 160 x 1008 image (its patch embedding is < 2 % of it)
    dp = Dims(canvas=160, canvas_w=1008)
    mp = model_from_dims(dp, dtype=dtype, max_batch=B, max_tokens=N)
    mp.load_state_dict(synth.synth_state_dict(dp, 0))
    v_ms = enc_ms(mp, torch.rand((B, 3, H, W), generator=g, device=dev, dtype=torch.float32))
    del mp
    torch.cuda.empty_cache()
    b_ms = max(e_ms - v_ms, 1e-3)
    fl = backbone_flop(B, H, W)
    # the bf16 engine keeps this backbone in fp32 STORAGE with fp32-accurate products: fp32 operands split hi + lo onto the bf16 matrix pipe
    # (csrc/gemm_split.h: three bf16 MFMAs per product term); the fp32 engine uses exact-f32 MFMA.  `achieved` counts the convolution's own
    # FLOPs once (fp32-equivalent); `peak` is the exact-f32 MFMA peak, the yardstick of an fp32 GEMM -- the split kernel may exceed it
    peak = 157.3
    tf = fl / (b_ms * 1e-3) / 1e12
    return {"value": round(B / sec, 2), "unit": "images/sec", "ms_per_step": round(1000 * sec, 3), "batch": B, "dtype": dtype,
            "workload": f"create_model(config.yml): hybrid ResNetV2 embedder, 1x{H}x{W} canvas, {N} tokens, greedy max_len={a.max_len}",
            "decode_path": "one persistent launch" if persistent else "one launch per stage",
            "encoder_ms": round(e_ms, 3), "vit_stack_ms": round(v_ms, 3), "backbone_ms": round(b_ms, 3),
            "backbone_mfma": {"achieved": round(tf, 1), "peak": peak, "unit": "TFLOP/s", "frac": round(tf / peak, 4),
                              "flop": fl, "arithmetic": ("fp32 storage; products as fp32 operands split onto the bf16 matrix pipe (~2^-16 per product)" if dtype == "bf16"
                                                        else "fp32 storage, exact-f32 MFMA") +
                                                       " -- bf16 storage moves these 45 random-weight layers by 10-20 % (tests/test_oracle_golden.py)"}}


def row_stop_measurement(dims, dtype, a, dev, B=256, target_median=90):
    """Per-row eos stop (stop='row', a build extension: SURVEY D7 / 8f N2) against the reference's global break on a SYNTHETIC eos
    schedule: random-init weights never produce eos, so to_logits.bias[eos] is raised until the median row finishes after about
    `target_median` tokens (bisection on the device; the schedule that results is reported).  Both runs decode the same rows to the
    same tokens up to each row's first eos (tests/test_gpu_stop.py); the global-break run keeps every row in every launch until the
    LAST row has finished, the row-stop run compacts the live rows of its row ranges every 16 positions."""
    import numpy as np
    import torch
    from texocr_amd import synth
    from texocr_amd.model import model_from_dims
    N = dims.n_tokens(a.height, a.width)
    m = model_from_dims(dims, dtype=dtype, max_batch=B, max_tokens=N)
    sd = synth.synth_state_dict(dims, 0)
    base = sd["decoder.net.to_logits.bias"].copy()
    g = torch.Generator(device=dev).manual_seed(777)
    img = torch.rand((B, dims.in_channels, a.height, a.width), generator=g, device=dev, dtype=torch.float32)
    img = img * torch.linspace(0.4, 1.6, B, device=dev)[:, None, None, None]          # rows differ: their eos positions spread

    def first_eos(bias):
        b = base.copy(); b[dims.eos] += bias
        sd["decoder.net.to_logits.bias"] = b
        m.load_state_dict(sd)
        t = m.generate(img, a.max_len).cpu().numpy()
        f = np.array([(np.nonzero(r == dims.eos)[0][0] + 1) if (r == dims.eos).any() else a.max_len + 1 for r in t])
        return f, t.shape[1]
    lo, hi = 0.0, 12.0
    for _ in range(10):
        mid = 0.5 * (lo + hi)
        f, _ = first_eos(mid)
        if np.median(f) > target_median: lo = mid
        else: hi = mid
    f, n_steps = first_eos(hi)

    def run(**kw):
        for _ in range(2): m.generate(img, a.max_len, **kw)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(5): out = m.generate(img, a.max_len, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / 5, out
    sec_g, out_g = run()
    sec_r, out_r = run(stop="row")
    comp = m._engine.query(5)
    same = bool(((out_g == out_r) | (out_r == dims.pad)).all().item()) and out_g.shape == out_r.shape
    res = {"batch": B, "dtype": dtype, "max_len": a.max_len, "eos_bias": round(hi, 3), "steps_decoded": int(n_steps),
           "row_lengths": {"median": float(np.median(f)), "mean": round(float(f.mean()), 1), "p90": float(np.percentile(f, 90)), "max": int(f.max()),
                           "rows_without_eos": int((f > a.max_len).sum())},
           "global_break": {"value": round(B / sec_g, 1), "unit": "images/sec", "ms_per_step": round(1000 * sec_g, 3)},
           "row_stop": {"value": round(B / sec_r, 1), "unit": "images/sec", "ms_per_step": round(1000 * sec_r, 3), "compactions": int(comp)},
           "speedup": round(sec_g / sec_r, 3), "tokens_agree_up_to_each_rows_eos": same,
           "note": "synthetic eos schedule (bias on the eos logit, random-init weights); global_break = the reference's loop (decoder.py:115-116)"}
    del m
    torch.cuda.empty_cache()
    return res


def side_measurement(dims, dtype, B, a, dev, warm, steps, want_cross, want_encoder, sampled=False):
    """One extra configuration on this GPU: throughput, and on request the cross-attention launch (HIP events bound to the
    dispatches of one generate) and the encoder span (marker events).  sampled: the reference's DEFAULT decode (top-k 99,
    temperature 0.3, one multinomial draw per step; ocr_model.py:47, decoder.py:104-108) instead of greedy."""
    import torch
    from texocr_amd import synth
    from texocr_amd.model import model_from_dims
    N = dims.n_tokens(a.height, a.width)
    m = model_from_dims(dims, dtype=dtype, max_batch=B, max_tokens=N)
    m.load_state_dict(synth.synth_state_dict(dims, 0))
    g = torch.Generator(device=dev).manual_seed(4321)
    img = torch.rand((B, dims.in_channels, a.height, a.width), generator=g, device=dev, dtype=torch.float32)
    m.eos_token = None if sampled else m.eos_token        # sampled rows may all hit eos early: keep the step at max_len positions
    sec = timed(m, img, a.max_len, warm, steps, **({"temp": 0.3, "decode": "sample", "seed": 1} if sampled else {}))
    out = {"value": round(B / sec, 2), "unit": "images/sec", "ms_per_step": round(1000 * sec, 3), "batch": B, "dtype": dtype, "steps": steps}
    esz = 2 if dtype == "bf16" else 4
    eng = m._engine

    def path_label():
        if eng.query(0) == 1:
            return "one persistent launch (csrc/persist.h), cross attention over projected K/V panels"
        form = "latent form (csrc/lat_attn.h: against the raw encoder rows)" if eng.query(3) == 1 else "projected K/V panels (csrc/dec_attn.h)"
        rng = eng.query(2)
        return (f"one launch per stage, {rng} row range{'s' if rng > 1 else ''} on {rng} stream{'s' if rng > 1 else ''}; cross attention: {form}")
    out["decode_path"] = path_label()
    if want_cross:
        # the cross-attention launch of ONE whole-batch range (profiling decodes on a single stream: with two row ranges the two
        # half-batch launches overlap each other and neither duration is the kernel's own)
        eng.profile(2)
        m.generate(img, a.max_len)
        torch.cuda.synchronize()
        ms, n = eng.profile_read(0)
        latent = eng.query(3) == 1
        eng.profile(0)
        algo_kv = B * dims.dec_heads * 2 * N * 64 * esz                     # K and V panels of every (image, head) once
        algo_lat = B * N * dims.embed_dim * esz                             # the raw encoder rows once for all heads (+ q', c: < 1 %)
        algo = algo_lat if latent else algo_kv
        ach = algo / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        out["roofline"] = {"kernel": ("lat_core_kernel (decode-step cross attention in latent form: scores and values against the raw encoder rows)" if latent
                                      else "dec_attn_kernel (decode-step cross-attention over projected K/V panels)"),
                           "timed_over": "a separate generate() with dispatch-bound HIP events on every fourth cross-attention launch; the profiling "
                                         "decode runs the whole batch as ONE row range on one stream (the throughput above: see decode_path)",
                           "bound": "hbm", "achieved": round(ach, 1),
                           "peak": 8000.0, "unit": "GB/s", "frac": round(ach / 8000.0, 4), "frac_of_achievable_6300": round(ach / 6300.0, 4),
                           "algorithmic_bytes_per_launch": algo, "algorithmic_bytes_kv_form": algo_kv, "algorithmic_bytes_latent_form": algo_lat,
                           "algorithmic_bytes": "the bytes of the form that ran (frac cannot exceed 1); kv_form = B*heads*2*N*64*s (SURVEY 8d), "
                                                "latent_form = B*N*D*s",
                           "kv_form_equivalent_GBps": round(algo_kv / (ms * 1e-3) / 1e9, 1) if ms > 0 else 0.0,
                           "avg_launch_us": round(ms * 1e3, 2), "launches_timed": n}
        try:        # PMC bytes of the same whole-batch launch from the separate rocprofv3 passes of probes/profile_r0N.sh (not measured in this run)
            fn = next(f for f in (os.path.join("profiles", f"{rnd}_pmc_{dtype}_b{B}" + ("" if latent or dims.embed_dim != 256 else "_kvform") + ".json")
                                  for rnd in ("r06", "r05")) if os.path.exists(os.path.join(ROOT, f)))
            pm = json.load(open(os.path.join(ROOT, fn)))["cross_attention_traffic"]
            if pm["config"] == {"batch": B, "dtype": dtype, "tokens": N} and pm.get("rows_per_launch") == B and ("lat_core" in pm["kernel"]) == latent and dims.embed_dim == 256:
                out["roofline"]["traffic"] = pm["traffic_bytes"]
                out["roofline"]["traffic_source"] = fn + " (separate rocprofv3 --pmc passes; not measured in this run)"
        except Exception:
            pass
        if B == 256 and latent and dims.embed_dim == 256 and dtype == "bf16" and "b256" in LIVE_PMC:
            out["roofline"]["traffic"] = LIVE_PMC["b256"]["traffic_bytes"]
            out["roofline"]["traffic_source"] = LIVE_PMC["b256"]["source"]
    if want_encoder:
        eng.profile(True)
        m.generate(img, a.max_len)
        torch.cuda.synchronize()
        ems, _ = eng.profile_read(1)
        eng.profile(False)
        peak = 2500.0 if dtype == "bf16" else 157.3
        tf = enc_flop(dims, B, N) / (ems * 1e-3) / 1e12 if ems > 0 else 0.0
        out["encoder_ms"] = round(ems, 3)
        out["encoder_mfma"] = {"achieved": round(tf, 1), "peak": peak, "unit": "TFLOP/s", "frac": round(tf / peak, 4)}
    del m
    torch.cuda.empty_cache()
    return out


def main():
    a = parse()
    if (not a.no_live_pmc and not a.no_roofline and a.model == "default" and "RANK" not in os.environ and a.gpus == 1):
        live_pmc(a)                                       # child processes: before this process initialises the GPU
    import torch
    import torch.distributed as dist
    from texocr_amd.config import Dims
    from texocr_amd import synth
    from texocr_amd.model import model_from_dims

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus and world > 1:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist_on = "RANK" in os.environ and "WORLD_SIZE" in os.environ      # launched by torch.distributed.run (also with one rank)
    if dist_on:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # RCCL prints a version banner on STDOUT when its first communicator comes up; stdout carries exactly ONE JSON line (the bench
        # contract), so the banner goes to stderr: file descriptor 1 points at 2 until the communicator exists
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
            warm = torch.zeros(8, device=dev)
            dist.all_reduce(warm)                       # the communicator (and its banner) now
            torch.cuda.synchronize()
        finally:
            sys.stdout.flush()
            os.dup2(saved_fd, 1)
            os.close(saved_fd)

    dims = Dims(canvas=max(a.height, a.width))          # config.yml dims, PatchEmbedding front end, C=3
    if a.model == "cfg4":
        dims = Dims(canvas=max(a.height, a.width), embed_dim=768, enc_heads=12, enc_layers=12, dec_heads=12, dec_layers=6)
    sd_np = synth.synth_state_dict(dims, 0)
    model = model_from_dims(dims, dtype=a.dtype, max_batch=a.batch, max_tokens=dims.n_tokens(a.height, a.width))
    model.load_state_dict(sd_np)
    eng = model._engine
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    imgs = [torch.rand((a.batch, dims.in_channels, a.height, a.width), generator=g, device=dev, dtype=torch.float32)
            for _ in range(2)]

    step = make_step(dist_on, lambda x, n: eng.generate(x, n, None), model.generate, imgs, a.max_len, dims.eos, dims.bos,
                     a.batch * world)

    if not a.no_roofline and rank == 0:
        eng.profile(3); eng.profile(2); eng.profile(0)          # creates the event pools now, outside the timed region
    t_settle = time.perf_counter()
    while time.perf_counter() - t_settle < a.settle_seconds:      # local work only: ranks may run different counts
        model.generate(imgs[0], a.max_len)
        torch.cuda.synchronize()
    for i in range(a.warmup):
        step(i)
    torch.cuda.synchronize()
    persistent = eng.query(0) == 1                  # which decode path generate() takes for this batch / dtype (engine.hip: persist_usable)
    if dist_on:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lat = []
    for i in range(a.steps):
        if i == a.steps - 1 and not a.no_roofline and rank == 0:
            # the LAST timed step carries HIP events bound to its dominant dispatch(es), nothing else on the stream:
            #   persistent decode (the default at this batch in bf16): the one launch of the whole decode loop;
            #   launch-per-stage decode: every fourth cross-attention dispatch (an event-carrying launch costs ~2 us of wall
            #   time: 9 % of a step with all of them instrumented, which `value` must not pay K times).
            eng.profile(3 if persistent else 2)
        s0 = time.perf_counter()
        out = step(i)
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - s0)
    torch.cuda.synchronize()
    if dist_on:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if dist_on:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    assert out.shape == (a.batch * world, a.max_len)

    result = None
    if rank == 0 and a.dump_outputs:
        dump_outputs(a.dump_outputs, {"tokens": out.cpu().numpy()})      # token ids < 2^24: exact in float32
    if rank == 0:
        lat.sort()
        N = dims.n_tokens(a.height, a.width)
        esz = 2 if a.dtype == "bf16" else 4
        result = {
            "metric": "images/sec (OCRModel.generate, greedy, max_len=256, 224x672 px)",
            "value": round(a.batch * world * a.steps / elapsed, 2), "unit": "images/sec",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(1000 * elapsed / a.steps, 3),
            "p50_latency_ms": round(1000 * lat[len(lat) // 2], 3),
            "p90_latency_ms": round(1000 * lat[min(len(lat) - 1, (9 * len(lat)) // 10)], 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": a.dtype, "data": "synthetic U[0,1) images, deterministic random-init weights (texocr_amd.synth seed 0)",
            "config": {"workload": ("BASELINE configs[1]: config.yml dims (256-d/8h/4L enc + 4L dec, patch 16, PatchEmbedding C=3), " if a.model == "default"
                                    else "BASELINE configs[3]: ViT-Base encoder (12L/768d/12h) + 6-layer decoder (768d/12h), PatchEmbedding C=3, ") +
                                   f"batch {a.batch}/GPU, {a.height}x{a.width}, greedy max_len={a.max_len}",
                       "global_batch": a.batch * world, "tokens_per_image": N,
                       "parallelism": f"dp{world} (images sharded, " + ("one RCCL all-gather of token ids per step" if dist_on else "single process, no collective") + ")",
                       "decode_path": "persistent launch (csrc/persist.h)" if persistent else
                                      (f"one launch per stage, {eng.query(2)} row range(s); cross attention in " + ("latent form" if eng.query(3) == 1 else "K/V form"))},
        }
        if not a.no_roofline:
            Ld, heads = dims.dec_layers, dims.dec_heads
            algo_cross = a.batch * heads * 2 * N * 64 * esz                 # one cross-attention launch / stage: K and V panels once
            mfma_peak = 2500.0 if a.dtype == "bf16" else 157.3              # dense TFLOP/s, MI355X_MICROARCH.md
            def pmc(kind):
                for rnd in ("r06", "r05", "r04", "r03", "r02", "r01"):
                    fn = os.path.join("profiles", f"{rnd}_pmc_{kind}{a.dtype}_b{a.batch}.json")
                    try:
                        pm = json.load(open(os.path.join(ROOT, fn)))["traffic"]
                        if pm["config"] == {"batch": a.batch, "dtype": a.dtype, "tokens": N, "max_len": a.max_len}:
                            return pm["traffic_bytes"], fn + " (separate rocprofv3 --pmc passes; not measured in this run)"
                    except Exception:
                        pass
                return None, None
            if persistent:
                ms_live, n_live = eng.profile_read(3)                       # the persistent launch of the last timed step
                # K/V bytes the decode loop has to read: per position, every layer, the cross panels (2*N rows) and the
                # self-attention history (2*(t+1) rows) of every (image, head), 64 elements each
                rows = sum(2 * N + 2 * (t + 1) for t in range(a.max_len))
                algo = a.batch * heads * 64 * esz * Ld * rows
                ach = algo / (ms_live * 1e-3) / 1e9 if ms_live > 0 else 0.0
                traffic, tsrc = pmc("persist_")
                if "persist" in LIVE_PMC:
                    traffic, tsrc = LIVE_PMC["persist"]["traffic_bytes"], LIVE_PMC["persist"]["source"]
                result["roofline"] = {
                    "kernel": "decode_persist_kernel (the whole 256-position decode loop as one launch; texocr_amd/csrc/persist.h)",
                    "bound": "hbm", "achieved": round(ach, 1), "peak": 8000.0, "unit": "GB/s", "frac": round(ach / 8000.0, 4),
                    "frac_of_achievable_6300": round(ach / 6300.0, 4),     # the same against the ~6.3 TB/s a streaming kernel reaches
                    "traffic": traffic, "traffic_source": tsrc, "algorithmic_bytes_per_launch": algo,
                    "algorithmic_bytes": "cross-attention K/V panels + self-attention history read once per position and layer "
                                         "(weights and activations stay in L2 / Infinity Cache): the bytes of the K/V FORM this kernel computes in",
                    # the latent form of the cross attention (csrc/lat_attn.h, what runs beyond 128 images) needs N*D instead of 2*N*heads*64
                    # elements per (image, layer, position): against THOSE bytes this launch is at frac_latent_form_bytes
                    "algorithmic_bytes_latent_form": a.batch * esz * Ld * sum(N * dims.embed_dim + 2 * (t + 1) * heads * 64 for t in range(a.max_len)),
                    "frac_latent_form_bytes": round(a.batch * esz * Ld * sum(N * dims.embed_dim + 2 * (t + 1) * heads * 64 for t in range(a.max_len))
                                                    / (ms_live * 1e-3) / 1e9 / 8000.0, 4) if ms_live > 0 else 0.0,
                    "avg_launch_us": round(ms_live * 1e3, 1), "launches_timed": n_live,
                    "timed_over": "the last of the K timed steps (HIP events bound to the dispatch)",
                    "us_per_position": round(ms_live * 1e3 / a.max_len, 2)}
            # the launch-per-stage path (what runs at other batch sizes / in fp32 / when profiling): cross-attention kernel by
            # dispatch-bound events of one generate, then encoder and whole-step spans by marker events
            os.environ["TXO_PERSIST"] = "0"
            try:
                eng.profile(2)
                model.generate(imgs[0], a.max_len)
                torch.cuda.synchronize()
                ms_x, n_x = eng.profile_read(0)
                lat_x = eng.query(3) == 1                               # beyond 128 images the launches run the cross attention in latent form
                eng.profile(True)
                model.generate(imgs[0], a.max_len)
                torch.cuda.synchronize()
                ems, en = eng.profile_read(1)
                sms, sn = eng.profile_read(2)
                eng.profile(False)
            finally:
                os.environ.pop("TXO_PERSIST")
            traffic, tsrc = None, None
            for rnd in ("r06", "r05", "r04", "r03", "r02", "r01"):
                fn = os.path.join("profiles", f"{rnd}_pmc_{a.dtype}_b{a.batch}.json")
                try:
                    pm = json.load(open(os.path.join(ROOT, fn)))["cross_attention_traffic"]
                    if pm["config"] == {"batch": a.batch, "dtype": a.dtype, "tokens": N}:
                        traffic, tsrc = pm["traffic_bytes"], fn + " (separate rocprofv3 --pmc passes; not measured in this run)"
                        break
                except Exception:
                    pass
            algo_kv_x = algo_cross
            if lat_x:
                algo_cross = a.batch * N * dims.embed_dim * esz             # latent form: the raw encoder rows once for all heads
                traffic, tsrc = None, None
            ach_x = algo_cross / (ms_x * 1e-3) / 1e9 if ms_x > 0 else 0.0
            cross = {"kernel": ("lat_core_kernel (decode-step cross attention in latent form, launch-per-stage path)" if lat_x else
                                "dec_attn_kernel (decode-step cross-attention, launch-per-stage path)"), "bound": "hbm",
                     "algorithmic_bytes_kv_form": algo_kv_x, "algorithmic_bytes_latent_form": a.batch * N * dims.embed_dim * esz,
                     "achieved": round(ach_x, 1), "peak": 8000.0, "unit": "GB/s", "frac": round(ach_x / 8000.0, 4), "frac_of_achievable_6300": round(ach_x / 6300.0, 4),
                     "traffic": traffic, "traffic_source": tsrc, "algorithmic_bytes_per_launch": algo_cross,
                     "avg_launch_us": round(ms_x * 1e3, 2), "launches_timed": n_x,
                     "timed_over": "a separate generate() with TXO_PERSIST=0 (dispatch-bound HIP events on every fourth launch)",
                     "decode_step_us_with_events": round(sms * 1e3, 1)}
            enc_tf = enc_flop(dims, a.batch, N) / (ems * 1e-3) / 1e12 if ems > 0 else 0.0
            enc = {"encoder_ms": round(ems, 3), "encoder_mfma": {"achieved": round(enc_tf, 1), "peak": mfma_peak, "unit": "TFLOP/s",
                                                                 "frac": round(enc_tf / mfma_peak, 4)}}
            if persistent:
                result["roofline"].update(enc)
                result["roofline_cross_attention_kernel"] = cross
            else:
                cross.update(enc)
                result["roofline"] = cross
        if "error" in LIVE_PMC:
            result["live_pmc_error"] = LIVE_PMC["error"]
        if world == 1 and not a.no_extras:
            del model, eng
            torch.cuda.empty_cache()
            try:
                result["fp32_parity_mode"] = side_measurement(dims, "fp32", a.batch, a, dev, 2, 5, False, False)
                result["fp32_parity_mode"]["note"] = "same workload on the token-exact fp32 engine (tests/test_gpu_parity.py pins it to the reference)"
                result["sampled_decode"] = side_measurement(dims, a.dtype, a.batch, a, dev, 2, 5, False, False, sampled=True)
                result["sampled_decode"]["note"] = ("same workload with the reference's default decode (decode='sample': top-k 99, temperature 0.3, "
                                                    "multinomial; eos test off so that all max_len positions run)")
                result["b256"] = side_measurement(dims, a.dtype, 256, a, dev, 2, 4, True, False)
                d4 = Dims(canvas=max(a.height, a.width), embed_dim=768, enc_heads=12, enc_layers=12, dec_heads=12, dec_layers=6)
                result["cfg4"] = side_measurement(d4, a.dtype, 256, a, dev, 1, 3, True, True)
                result["cfg4"]["workload"] = "BASELINE configs[3]: ViT-Base encoder (12L/768d/12h) + 6-layer decoder (768d/12h), batch 256"
                result["cfg5_beam"] = beam_measurement(a.dtype, a, dev)
                result["cfg5_beam"]["parity"] = "unpinned beyond k=1: the reference has no beam search (checked against the oracle's own beam search only)"
                result["row_stop_b256"] = row_stop_measurement(dims, a.dtype, a, dev)
                result["hybrid_default"] = hybrid_measurement(a.dtype, a, dev)
            except Exception as e:                          # a side measurement must never lose the headline line
                result["extras_error"] = f"{type(e).__name__}: {e}"
        if not a.no_cpu_baseline and world == 1:            # reported at N=1 only (bench contract)
            result["cpu_baseline"] = cpu_baseline(dims, sd_np, a)
        print(json.dumps(result), flush=True)
    if dist_on:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
