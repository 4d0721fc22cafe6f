"""What the GPU tests share (tests/test_gpu_*.py import it like ref64 and sampler_ref; it holds no tests and no bounds of its own except
the calibrated bf16 bound two modules assert): building an engine, the TXO_* knobs around a call, the two decode paths with the
assertion of which one ran, the reference-fixture set-ups several modules repeat, and the cases more than one module decodes.

This is the only test-side file that touches os.environ.  Engines are built per test: nothing here caches one."""
import contextlib
import os

import numpy as np
import torch

from texocr_amd import synth
from texocr_amd._lib import Q_LAST_PERSISTENT, Q_PERSIST_FALLBACKS
from texocr_amd.config import Dims


def oracle():
    from oracle import cpu_ref
    return cpu_ref


@contextlib.contextmanager
def knobs(**kv):
    """TXO_* variables around calls; on exit the values of entry are put back.  TXO_PERSIST / TXO_LANES / TXO_GRAPH / TXO_NET_STEPWISE
    are re-read by the binding whenever the environment changes between two calls on a live engine; what the engine reads once, when
    it is created (TXO_LATENT, TXO_LAT_G, the TXO_STOP_* periods, ...), goes through build(env=...)."""
    before = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def build(meta_or_dims, seed=None, dtype="fp32", max_batch=8, max_tokens=0, latent=None, sd=None, env=None):
    """latent: None = the engine's default choice of the cross-attention form; 0 / 1 = the projected K/V panels / the raw encoder
    rows (csrc/lat_attn.h) on every decode with launches (TXO_LATENT, read once when the engine is created).
    env: further knobs the engine reads once at creation (TXO_LAT_G, TXO_LATENT_SELF, ...)."""
    from texocr_amd.model import model_from_dims
    if isinstance(meta_or_dims, dict):
        d, seed = Dims(**meta_or_dims["dims"]), meta_or_dims["weight_seed"]
    else:
        d = meta_or_dims
    sd = sd if sd is not None else synth.synth_state_dict(d, seed)
    create = dict(env or {})
    if latent is not None:
        create["TXO_LATENT"] = int(latent)
    with knobs(**create):
        m = model_from_dims(d, dtype=dtype, max_batch=max_batch, max_tokens=max_tokens)
    m.load_state_dict(sd)
    return d, sd, m


def images(meta):
    return torch.from_numpy(synth.synth_images(*meta["image_shape"], seed=meta["image_seed"]))


def rgb_images(b, h, w, seed):
    return torch.from_numpy(synth.synth_images(b, 3, h, w, seed=seed))


def fixture_rows_in_batch(meta, batch, rows, seed):
    """the fixture's images as rows `rows` of a random batch of their size (rows never interact; decoder.py:115 is the only cross-row
    operation), on the GPU"""
    fix = images(meta).cuda()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    img = torch.rand((batch, *fix.shape[1:]), generator=gen, device="cuda")
    for r, f in zip(rows, fix):
        img[r] = f
    return img


def assert_tokens_exact_up_to_margin(tok, ref_tok, ref_logits, thr=2e-5):
    """tokens must be identical until (per row) the first step whose oracle top1-top2 margin < thr."""
    top2 = ref_logits.topk(2, dim=-1).values
    margin = (top2[..., 0] - top2[..., 1]).numpy()
    for b in range(tok.shape[0]):
        small = np.nonzero(margin[b] < thr)[0]
        upto = int(small[0]) if small.size else tok.shape[1]
        assert np.array_equal(tok[b, :upto], ref_tok[b, :upto]), (b, upto)


def per_image_rel(enc, ref, scale=None):
    """(B,) mean |enc - ref| over an image's tokens and columns / mean |scale| of that image (scale: ref unless given).  The hybrid tests
    assert its MAXIMUM over a batch: a batch mean hides one image's wrong GroupNorm statistics behind a weight of 1 / B."""
    enc, ref = torch.as_tensor(enc).double().cpu(), torch.as_tensor(ref).double().cpu()
    scale = ref if scale is None else torch.as_tensor(scale).double().cpu()
    return (enc - ref).abs().mean(dim=(1, 2)) / scale.abs().mean(dim=(1, 2))


def top5_error(logits, g, upto=None):
    """max |logits - reference| over the reference's top-5 of every position (fixture arrays top5_ids / top5_vals; the first `upto`
    positions); logits (B, n, V) on the host"""
    ids, vals = g["top5_ids"][:, :upto], g["top5_vals"][:, :upto]
    got = torch.gather(logits, 2, torch.from_numpy(ids.astype(np.int64)))
    return float((got - torch.from_numpy(vals)).abs().max())


def top5_error_and_top1_agreement(logits, toks, g, upto=None):
    """teacher-forced logits against a reference fixture: (top5_error, fraction of positions whose arg-max is the reference's token)"""
    return top5_error(logits, g, upto), float((logits.argmax(-1) == toks).float().mean())


def teacher_forced_stepwise(m, d, img, ref_tokens):
    """decoder.net() as single-position steps (TXO_NET_STEPWISE=1): the reference's tokens fed through the DECODE kernels of the
    launch path (dec_gemm / dec_attn or lat_attn), every position's logits"""
    toks = torch.from_numpy(ref_tokens.astype(np.int64)).cuda()
    prefix = torch.cat([torch.full((toks.shape[0], 1), d.bos, dtype=torch.long, device="cuda"), toks[:, :-1]], 1)
    with knobs(TXO_NET_STEPWISE=1):
        return m.decoder.net(prefix, enc=m.encoder(img)).cpu(), toks.cpu()


def on_path(m, persistent, call):
    """call() with the decode forced through the persistent launch (TXO_PERSIST=1) or through launches (0); asserts that this path
    ran and that no persistent launch of the engine has fallen back"""
    with knobs(TXO_PERSIST=int(persistent)):
        out = call()
    assert m._engine.query(Q_LAST_PERSISTENT) == int(persistent), f"TXO_PERSIST={int(persistent)}: the other decode path ran"
    assert m._engine.query(Q_PERSIST_FALLBACKS) == 0, "a persistent launch fell back to launches"
    return out


def both_paths(m, img, max_len, **kw):
    """generate() through the persistent launch and through launches: (persistent result, launch result)"""
    return tuple(on_path(m, p, lambda: m.generate(img, max_len, **kw)) for p in (True, False))


# ---- per-row stop (tests/test_gpu_stop.py; the shape matrix and the sampler tests decode the same case) -----------------------------
STOP_ENV = {"TXO_STOP_EVERY": "2", "TXO_STOP_GAIN": "1"}          # a compaction every other position (read when the engine is created)

STOP_DIMS = Dims(canvas=64, in_channels=3, embed_dim=64, enc_heads=2, enc_layers=2, dec_heads=2, dec_layers=2, vocab=64, max_len=48,
                 bos=62, eos=61, pad=63)


def first_eos(tok, eos):
    return [int(np.nonzero(r == eos)[0][0]) if (r == eos).any() else -1 for r in tok]


def stop_case(rows=40, bias=1.2):
    """40 tiny images of different contrast, eos favoured by a logit bias: rows produce their first eos anywhere between position 0
    and 46, some never (tuned on the oracle; its smallest top-1/top-2 margin is 5e-4, a hundred times the fp32 error)."""
    d = STOP_DIMS
    sd = synth.synth_state_dict(d, 7)
    b = sd["decoder.net.to_logits.bias"].copy()
    b[d.eos] += bias
    sd["decoder.net.to_logits.bias"] = b
    img = torch.from_numpy(synth.synth_images(rows, 3, 32, 48, seed=11)) * torch.linspace(0.2, 3.0, rows)[:, None, None, None]
    return d, sd, img


# ---- the shape matrix (tests/test_gpu_shapes.py; the sampler tests take their widths and the bf16 bound from it) --------------------
def _shape_dims(D, eh, dh, ee, de, vocab):
    return Dims(canvas=128, in_channels=3, embed_dim=D, enc_heads=eh, enc_layers=1, dec_heads=dh, dec_layers=2, enc_exp=ee, dec_exp=de,
                vocab=vocab, max_len=32, bos=vocab - 2, eos=vocab - 3, pad=vocab - 1)


# name: (dims, what it reaches)
SHAPE_CASES = {
    "w64_h4": (_shape_dims(64, 4, 4, 1, 1, 200), "inner 256 > D, GeGLU width 64, latent core at D = 64 with 4 heads"),
    "w128": (_shape_dims(128, 2, 2, 4, 4, 200), "ln_rows_generic_kernel; fp32 dec_gemm KW = 2 (K = 128); bf16 run-time K, one k-chunk per wave"),
    "w192_h3": (_shape_dims(192, 3, 3, 2, 1, 333), "bf16 K = 192: 6 k-chunks split 2/2/1/1 over the waves, A-swizzle mask 7; odd vocabulary"),
    "w256_h3": (_shape_dims(256, 5, 3, 1, 3, 1000), "latent at 256 with 3 decoder heads (bf16: the 4-wave tile); no persistent kernel; "
                                              "out-projection K = 192"),
    "w384_h6": (_shape_dims(384, 6, 6, 4, 4, 1000), "ViT-Small-like; fp32 dec_gemm KW = 6 (K = 384), bf16 run-time K = 384; two row ranges "
                                              "on the K/V form at 130 bf16 rows"),
    "w512": (_shape_dims(512, 8, 8, 4, 2, 1000), "ln_rows_kernel<., 2>; bf16 >= 128 rows: LayerNorm launch + GEMM for the FFN-in"),
    "w704_h11": (_shape_dims(704, 11, 11, 3, 3, 1000), "largest generic LayerNorm (11 float4 per lane); bf16 22 k-chunks"),
    "w768_h20": (_shape_dims(768, 20, 20, 1, 1, 1000), "heads > 16: two latent tiles per row, beam packing across tiles; dec_gemm_wide_kernel; "
                                                 "no persistent kernel"),
    "calib256": (_shape_dims(256, 8, 8, 4, 4, 1000), "config.yml widths (persistent launch): calibrates the bf16 bounds"),
    "calib768": (_shape_dims(768, 12, 12, 4, 4, 1000), "ViT-Base widths: calibrates the bf16 bounds"),
}

# bf16 against float64 (2 decoder layers, 24 steps, IMAGE_SETS and BF16_ROWS of test_gpu_shapes.py), max |d| measured on MI355X:
#   calib256: encoder 0.0198, logits teacher forced 0.0371 / greedy 0.0323 (latent form 0.0322)
#   calib768: encoder 0.0199, logits teacher forced 0.0314 / greedy 0.0299 (latent form 0.0327)
# the new widths sit at encoder 0.019-0.024 and logits 0.030-0.041 (w64_h4 teacher forced); a wrong index gives 1-4
BF16_CALIB = {"enc": 0.0199, "logits": 0.0371}
BF16_BOUND = {k: 1.5 * v for k, v in BF16_CALIB.items()}
