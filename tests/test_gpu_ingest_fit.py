"""Fit-to-canvas ingest on the GPU (txo_ingest_u8_fit, texocr_amd/csrc/ingest_fit.h): an oversized image is downscaled on the device to the
very bytes PIL's BILINEAR resize gives, so the container equals tests/fit_ref.py -> the host preprocessing bit for bit, and everything
downstream is identical by either ingest.  Sources and PIL's answers come from tests/golden/fit_cases.npz (tests/test_ingest_fit_cpu.py pins
fit_ref to them without a GPU); only the end-to-end test, whose host path IS a call into PIL, needs PIL."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import fit_ref
import ingest_cases
from gpu_harness import knobs
from texocr_amd import synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _wrapper(tmp, img_size, dtype="fp32", max_batch=3):
    from texocr_amd.config import default_config
    from texocr_amd.tokenizer import RegExTokenizer
    from texocr_amd.wrapper import TeXOCRWrapper
    v = json.load(open(os.path.join(GOLDEN, "tokenizer_vocab_1k.json")))
    path = str(tmp / "vocab.txt")
    RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"]).save(path)
    cfg = default_config(img_size=list(img_size), max_length=32, in_channels=1,
                         encoder={"embed_dim": 64, "heads": 2, "num_layers": 1}, decoder={"embed_dim": 64, "heads": 2, "num_layers": 2})
    cfg["tokenizer_path"] = path
    w = TeXOCRWrapper(cfg, dtype=dtype, max_batch=max_batch)
    w.model.load_state_dict(synth.synth_state_dict(w.dims, 5))
    return w


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """the tiny model on a 32 x 96 canvas: the target of the fixture's batch; max_batch holds all of it"""
    return _wrapper(tmp_path_factory.mktemp("fit"), (32, 96), max_batch=16)


@pytest.fixture(scope="module")
def cases():
    z = np.load(os.path.join(GOLDEN, "fit_cases.npz"))
    meta = {c["name"]: c for c in json.load(open(os.path.join(GOLDEN, "fit_cases.json")))["cases"]}
    return {name: (z["src_" + name], c) for name, c in meta.items()}


def _batch(cases, target):
    return [a for a, c in cases.values() if (c["Fh"], c["Fw"]) == target]


def _reference(arrs, Fh, Fw, channels):
    """fit_ref -> the host preprocessing (ingest_cases.kernel_steps is preprocess_image's arithmetic, tests/test_ingest_cpu.py) -> the
    container and the sizes pack_ragged would build"""
    fitted = [fit_ref.fit(a, Fh, Fw) for a in arrs]
    sizes = torch.tensor([[(f.shape[0] + 15) // 16 * 16, (f.shape[1] + 15) // 16 * 16] for f in fitted], dtype=torch.int32)
    box = torch.zeros((len(arrs), channels, int(sizes[:, 0].max()), int(sizes[:, 1].max())), dtype=torch.float32)
    for b, f in enumerate(fitted):
        box[b, :, :f.shape[0], :f.shape[1]] = torch.from_numpy(ingest_cases.kernel_steps(f))
    return box, sizes, fitted


def _pack(w, arrs, channels, fit):
    from texocr_amd import ops
    with knobs(TXO_DEBUG_POISON=1):                                # the output starts as NaN: an element left unwritten fails torch.equal
        got = ops.pack_u8(arrs, channels, torch.device("cuda", 0), engine=w.model._engine.id, fit=fit)
    box = got.box.cpu()
    assert not torch.isnan(box).any(), "an element of the container was left unwritten"
    return box, got.sizes


# ---- 1. container bit-identity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
def test_mixed_batch_container_is_bit_identical(small, cases, channels):
    """images that fit (1x1, 16x16, 32x96, 20x50) and oversized ones (33x96, 32x97, 64x192, 47x301, 70x500 RGBA, 1x400, 300x1, 1024x3072 at
    scale 32 on both axes, 2x3000 whose height clamps to 1) in ONE call, L / RGB / RGBA mixed"""
    arrs = _batch(cases, (32, 96))
    assert len(arrs) == 13 and {a.shape[2] if a.ndim == 3 else 1 for a in arrs} == {1, 3, 4}
    ref_box, ref_sizes, fitted = _reference(arrs, 32, 96, channels)
    assert sum(f is not a for f, a in zip(fitted, arrs)) == 9 and tuple(ref_box.shape) == (13, channels, 32, 96)
    box, sizes = _pack(small, arrs, channels, (32, 96))
    assert torch.equal(sizes, ref_sizes) and sizes.dtype == torch.int32 and not sizes.is_cuda
    assert tuple(box.shape) == tuple(ref_box.shape)
    bad = [(b, int((box[b] != ref_box[b]).sum())) for b in range(len(arrs)) if not torch.equal(box[b], ref_box[b])]
    assert not bad, bad
    # model.ingest(fit=True) is the same call with the model's canvas and in_channels
    got = small.model.ingest(arrs, fit=True)
    assert torch.equal(got.sizes, ref_sizes) and torch.equal(got.box.cpu(), _reference(arrs, 32, 96, 1)[0])


# ---- 2. value coverage -------------------------------------------------------------------------------------------------------------------
def test_every_byte_value_and_the_clamp(small, cases):
    """64x512 under the target (16, 16): 0 meets 255 inside every tap window and every byte value occurs; all-255 images must come out as
    exactly 255 per pixel before the luma (the coefficients' sum may exceed 2^22: the clamp matters)"""
    arrs = _batch(cases, (16, 16))
    assert len(arrs) == 3 and len(np.unique(cases["coverage_64x512"][0])) == 256
    ref_box, ref_sizes, fitted = _reference(arrs, 16, 16, 1)
    box, sizes = _pack(small, arrs, 1, (16, 16))
    assert torch.equal(sizes, ref_sizes) and torch.equal(box, ref_box), int((box != ref_box).sum())
    white = float(ingest_cases.kernel_steps(np.full((1, 1), 255, np.uint8))[0, 0])
    for b in (1, 2):                                               # white_64x512 (L), white_rgb_40x130
        fh, fw = fitted[b].shape[:2]
        assert int(fitted[b].min()) == 255 and bool((box[b, 0, :fh, :fw] == white).all()) and white != 0.0
        assert not box[b, 0, fh:].any() and not box[b, 0, :, fw:].any()


# ---- 3. nothing oversized: txo_ingest_u8's container, no scratch -------------------------------------------------------------------------
def test_no_oversized_image_equals_ingest_u8(small, cases):
    from texocr_amd import ops
    arrs = [a for a, c in cases.values() if (c["h"], c["w"]) == (c["fh"], c["fw"]) and (c["Fh"], c["Fw"]) == (32, 96)]
    rng = np.random.RandomState(2)
    arrs += [rng.randint(0, 256, shape).astype(np.uint8) for shape in ((15, 16, 3), (17, 33, 4), (32, 95), (9, 96, 3))]
    assert len(arrs) == 8
    need = C.c_int64(-1)
    shapes = ops.plan_u8(arrs)[3]
    assert small.model._engine.lib.txo_ingest_fit_scratch(ops._i32p(shapes), len(arrs), 32, 96, C.byref(need)) == 0
    assert need.value == 0                                         # so the operator passes a NULL scratch
    box, sizes = _pack(small, arrs, 1, (32, 96))
    ref_box, ref_sizes = _pack(small, arrs, 1, None)
    assert torch.equal(sizes, ref_sizes) and torch.equal(box, ref_box)


# ---- 4. device-resident inputs at an odd byte offset ---------------------------------------------------------------------------------------
def test_device_resident_images_at_odd_offsets(small, cases):
    arrs = [cases[n][0] for n in ("over_47x301", "fits_20x50", "over_70x500", "over_33x96", "over_300x1")]
    ref_box, ref_sizes, _ = _reference(arrs, 32, 96, 1)
    dev = []
    for k, a in enumerate(arrs):
        buf = torch.zeros((a.size + 3,), dtype=torch.uint8, device="cuda")
        off = 1 + 2 * (k % 2)                                      # 1 or 3: never a multiple of 2
        buf[off:off + a.size] = torch.from_numpy(a.reshape(-1)).cuda()
        t = buf[off:off + a.size].view(a.shape)
        assert t.is_contiguous() and t.data_ptr() % 2 == 1
        dev.append(t)
    box, sizes = _pack(small, dev, 1, (32, 96))
    assert torch.equal(sizes, ref_sizes) and torch.equal(box, ref_box)
    mixed = [dev[k] if k % 2 else arrs[k] for k in range(len(arrs))]                    # host and device images in one list
    box, sizes = _pack(small, mixed, 1, (32, 96))
    assert torch.equal(sizes, ref_sizes) and torch.equal(box, ref_box)


# ---- 5. refusals reach Python; the default still refuses -------------------------------------------------------------------------------------
def test_refusals_reach_python(small):
    from texocr_amd import ops
    eng = small.model._engine
    good = np.zeros((20, 40, 3), np.uint8)
    with pytest.raises(ValueError, match=r"ingest: image 1 is 3x5000, 1x96 fitted to 32x96: an axis shrinks by more than 32 times"):
        small.model.ingest([good, np.zeros((3, 5000), np.uint8)], fit=True)
    with pytest.raises(ValueError, match="the fit target is 32x100; both sides must be positive multiples of 16"):
        ops.pack_u8([good], 1, torch.device("cuda", 0), engine=eng.id, fit=(32, 100))
    staged, dev, src, shapes = ops.plan_u8([good, np.zeros((47, 301), np.uint8)])
    with pytest.raises(ValueError, match=r"image 1 is 14x96, 16x96 rounded up to multiples of 16: it does not fit the container's 32x80"):
        torch.ops.texocr.ingest_u8_fit([staged.cuda()], src, shapes, eng.id, 1, 32, 96, 32, 80)
    # ... and the engine is as it was
    box, sizes = torch.ops.texocr.ingest_u8_fit([staged.cuda()], src, shapes, eng.id, 1, 32, 96, 32, 96)
    assert sizes.tolist() == [[32, 48], [16, 96]] and torch.equal(box[1, 0, :14], torch.ones((14, 96), device="cuda"))


# ---- 6. end to end -------------------------------------------------------------------------------------------------------------------------
def _pil_list():
    """four images for the 64 x 256 canvas, two of them oversized (100x600 RGB: the width binds; 150x200 L: the height binds)"""
    from PIL import Image
    rng = np.random.RandomState(0)
    pil = []
    for k, (wd, ht) in enumerate([(200, 40), (600, 100), (30, 30), (200, 150)]):
        a = np.full((ht, wd, 3), 255, dtype=np.uint8)
        a[rng.randint(0, ht, 300), rng.randint(0, wd, 300)] = rng.randint(0, 120, (300, 3 if k % 2 else 1))
        pil.append(Image.fromarray(a) if k != 3 else Image.fromarray(a).convert("L"))
    return pil


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y)
        for u, v in zip(x, y):
            assert torch.equal(u, v) if isinstance(u, torch.Tensor) else u == v, (u, v)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_batch_and_call_agree_by_either_ingest(tmp_path, dtype):
    """fit='canvas': tokens, LaTeX, log-probabilities and maps are identical by either ingest -- greedy, seeded sampling, beam, align -- over a
    list longer than max_batch with two oversized images; fit='none' keeps refusing the list; the maps are on the fitted grid"""
    w = _wrapper(tmp_path, (64, 256), dtype=dtype, max_batch=3)
    pil = _pil_list()
    fitted = [fit_ref.fit_size(im.size[1], im.size[0], 64, 256) for im in pil]
    assert fitted == [(40, 200), (42, 256), (30, 30), (64, 85)]
    for kw in (dict(decode="greedy", return_logp=True), dict(decode="sample", seed=11, return_logp=True), dict(decode="beam", beams=3, return_logp=True),
               dict(decode="greedy", return_align=True)):
        host = w.batch(pil, max_len=12, ingest="host", fit="canvas", **kw)
        dev = w.batch(pil, max_len=12, ingest="device", fit="canvas", **kw)
        assert len(host) == len(pil) > w.model._engine.max_batch
        _same(host, dev)
        if kw.get("return_align"):
            for (toks, _, maps), (fh, fw) in zip(dev, fitted):
                assert tuple(maps.shape) == (len(toks), (fh + 15) // 16, (fw + 15) // 16)
    for im in pil[1:3]:
        _same([w(im, max_len=12, decode="greedy", return_logp=True, return_align=True, fit="canvas")],
              [w(im, max_len=12, decode="greedy", return_logp=True, return_align=True, fit="canvas", ingest="device")])
    # an image that fits is untouched by the switch
    _same(w.batch(pil[::2], max_len=12, decode="greedy", fit="canvas", ingest="device"), w.batch(pil[::2], max_len=12, decode="greedy"))
    # every default keeps today's refusal of the oversized images, by either ingest
    for ingest in ("host", "device"):
        with pytest.raises(ValueError, match="ragged batches: image 1 is larger than the position-embedding canvas"):
            w.batch(pil, max_len=12, decode="greedy", ingest=ingest)
        with pytest.raises(ValueError, match="ragged batches: image 1 is larger than the position-embedding canvas"):
            w.batch(pil, max_len=12, decode="greedy", ingest=ingest, fit="none")
        with pytest.raises(ValueError, match="image size 112x608 exceeds the 64x256 canvas"):
            w(pil[1], max_len=12, decode="greedy", ingest=ingest)
    with pytest.raises(ValueError, match="fit must be 'none' or 'canvas'"):
        w.batch(pil, fit="crop", ingest="device")


# ---- the torch-free route --------------------------------------------------------------------------------------------------------------
def test_torch_free_c_program_fits_an_oversized_image(tmp_path):
    """examples/ingest_fit_tiny.c: plain C + the HIP runtime API: txo_ingest_fit + txo_ingest_box + txo_ingest_fit_scratch + txo_ingest_u8_fit +
    txo_generate_ragged; its container must equal the resample (over txo_ingest_fit_coeffs' table) and preprocessing done in C on the host,
    and the fitted sizes it prints are the Python rule's"""
    import subprocess
    import sys
    from texocr_amd import build as b, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = b.build_example(verbose=False, name="ingest_fit_tiny")
    blob = str(tmp_path / "tiny.bin")
    subprocess.run([sys.executable, os.path.join(root, "examples", "make_tiny_blob.py"), blob], check=True, capture_output=True)
    r = subprocess.run([exe, blob], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "equals the host resample and preprocessing bit for bit" in r.stdout and "equal the host container's" in r.stdout
    assert "-> -1 (ingest: image 1 is" in r.stdout and "an axis shrinks by more than 32 times" in r.stdout
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("fit to ")][0]          # "fit to FhxFw: hxw -> h'xw', ..."
    Fh, Fw = (int(v) for v in line.split(":")[0][len("fit to "):].split("x"))
    pairs = [p.strip().split(" -> ") for p in line.split(":")[1].split(",")]
    assert len(pairs) == 3
    for src, dst in pairs:
        h, wd = (int(v) for v in src.split("x"))
        assert ops.fit_size(h, wd, Fh, Fw) == tuple(int(v) for v in dst.split("x")), line
    assert any(src != dst for src, dst in pairs)
