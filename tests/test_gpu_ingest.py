"""Device-side image ingest on the GPU (txo_ingest_u8, texocr_amd/csrc/ingest.h): the container it writes is bit for bit the one the host
path ends in -- pack_ragged([wrapper._tensor(im) for im in imgs]) -- so nothing downstream may differ: TeXOCRWrapper.batch / __call__ by
either ingest, the fixed-shape calls on an ingested box, the opt-in hybrid front end; and the engine's refusals reach Python.  The image
lists are tests/ingest_cases.py (tests/test_ingest_cpu.py pins the arithmetic on them without a GPU)."""
import json
import os

import numpy as np
import pytest
import torch

import ingest_cases as cases
from gpu_harness import knobs
from texocr_amd import synth

pytestmark = pytest.mark.gpu


def _wrapper(tmp, in_channels=1, dtype="fp32", max_batch=3, **kw):
    from texocr_amd.config import default_config
    from texocr_amd.tokenizer import RegExTokenizer
    from texocr_amd.wrapper import TeXOCRWrapper
    v = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tokenizer_vocab_1k.json")))
    path = str(tmp / "vocab.txt")
    RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"]).save(path)
    cfg = default_config(img_size=kw.pop("img_size", [64, 256]), max_length=32, in_channels=in_channels,
                         encoder={"embed_dim": 64, "heads": 2, "num_layers": 1}, decoder={"embed_dim": 64, "heads": 2, "num_layers": 2}, **kw)
    cfg["tokenizer_path"] = path
    w = TeXOCRWrapper(cfg, dtype=dtype, max_batch=max_batch, ragged_hybrid=kw.get("embed") == "hybrid")
    w.model.load_state_dict(synth.synth_state_dict(w.dims, 5))
    return w


@pytest.fixture(scope="module")
def wrappers(tmp_path_factory):
    """the tiny test model with one and with three input channels (fp32); max_batch holds the longest list of the container tests"""
    tmp = tmp_path_factory.mktemp("ingest")
    return {c: _wrapper(tmp, in_channels=c, max_batch=18) for c in (1, 3)}


def _as_device_tensors(imgs):
    """the same bytes as uint8 tensors that already lie on the device; every third one is NOT contiguous (pack_u8 makes it so)"""
    out = []
    for k, im in enumerate(imgs):
        a = torch.from_numpy(np.array(im)).cuda()
        if k % 3 == 2:
            wide = torch.zeros((a.shape[0], a.shape[1] + 5, *a.shape[2:]), dtype=torch.uint8, device="cuda")
            wide[:, :a.shape[1]] = a
            a = wide[:, :a.shape[1]]
            assert not a.is_contiguous()
        out.append(a)
    return out


# ---- 1. container bit-identity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [False, True], ids=["pil", "device_u8"])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("name", ["mixed_list", "sweep_list", "flat_list"])
def test_container_is_bit_identical_to_the_host_path(wrappers, name, channels, resident):
    from texocr_amd import ops
    w = wrappers[channels]
    imgs = getattr(cases, name)()
    ref_box, ref_sizes = ops.pack_ragged([w._tensor(im) for im in imgs])
    with knobs(TXO_DEBUG_POISON=1):                                # the output starts as NaN: an element left unwritten fails torch.equal
        got = w.model.ingest(_as_device_tensors(imgs) if resident else imgs)
    assert isinstance(got, ops.PackedImages) and got.box.is_cuda and got.box.dtype == torch.float32
    assert torch.equal(got.sizes, ref_sizes) and got.sizes.dtype == torch.int32 and not got.sizes.is_cuda
    box = got.box.cpu()
    assert tuple(box.shape) == tuple(ref_box.shape)
    assert not torch.isnan(box).any(), "an element of the container was left unwritten"
    assert torch.equal(box, ref_box), int((box != ref_box).sum())
    if name == "flat_list":                                        # pad pixels are 0.0, not the value white maps to
        white = float(cases.kernel_steps(np.full((1, 1), 255, np.uint8))[0, 0])
        for b, im in enumerate(imgs):
            h, wd = np.asarray(im).shape[:2]
            inside = box[b, :, :h, :wd]
            assert bool((inside == (white if np.asarray(im).max() == 255 else 1.0)).all()), b
            assert white != 0.0 and not box[b, :, h:].any() and not box[b, :, :, wd:].any(), b


def test_numpy_and_mixed_residency_in_one_list(wrappers):
    """host arrays and device tensors in ONE list: the host ones travel in the staged buffer, the device ones are read where they lie"""
    from texocr_amd import ops
    w = wrappers[1]
    imgs = cases.mixed_list()[:9]
    ref_box, ref_sizes = ops.pack_ragged([w._tensor(im) for im in imgs])
    dev = _as_device_tensors(imgs)
    mixed = [dev[k] if k % 2 else (np.array(im) if k % 4 else im) for k, im in enumerate(imgs)]
    with knobs(TXO_DEBUG_POISON=1):
        got = w.model.ingest(mixed)
    assert torch.equal(got.box.cpu(), ref_box) and torch.equal(got.sizes, ref_sizes)


# ---- 2. end to end -----------------------------------------------------------------------------------------------------------------
def _pil_list():
    from PIL import Image
    rng = np.random.RandomState(0)
    pil = []
    for k, (wd, ht) in enumerate([(200, 40), (30, 30), (250, 64), (100, 17)]):
        a = np.full((ht, wd, 3), 255, dtype=np.uint8)
        a[rng.randint(0, ht, 40), rng.randint(0, wd, 40)] = rng.randint(0, 120, (40, 3 if k % 2 else 1))
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
    """the containers are equal, so tokens, LaTeX, log-probabilities and maps are: greedy, sampled, beam, prefix, align -- over a list
    longer than max_batch (two chunks)"""
    w = _wrapper(tmp_path, dtype=dtype, max_batch=3)
    pil = _pil_list()
    for kw in (dict(decode="greedy", return_logp=True), dict(decode="sample", seed=11, return_logp=True), dict(decode="beam", beams=3, return_logp=True),
               dict(decode="greedy", prefix=[r"\frac", [5, 6], "x", r"\begin{aligned}"], return_logp=True), dict(decode="greedy", return_align=True)):
        host = w.batch(pil, max_len=12, ingest="host", **kw)
        dev = w.batch(pil, max_len=12, ingest="device", **kw)
        assert len(host) == len(pil) > w.model._engine.max_batch
        _same(host, dev)
    assert w.batch(pil, max_len=12, decode="greedy") == w.batch(pil, max_len=12, decode="greedy", ingest="device")   # the default is 'host'
    for im in pil[:2]:
        _same([w(im, max_len=12, decode="greedy", return_logp=True, return_align=True)],
              [w(im, max_len=12, decode="greedy", return_logp=True, return_align=True, ingest="device")])
    with pytest.raises(ValueError, match="ingest must be 'host' or 'device'"):
        w.batch(pil, ingest="gpu")


# ---- 3. fixed shape ----------------------------------------------------------------------------------------------------------------
def test_box_of_equal_sizes_is_a_fixed_shape_batch(wrappers):
    from PIL import Image
    w = wrappers[3]
    rng = np.random.RandomState(4)
    imgs = [Image.fromarray(rng.randint(0, 256, (30, 70, 3)).astype(np.uint8)) for _ in range(3)]
    stacked = torch.stack([w._tensor(im) for im in imgs]).cuda()
    box = w.model.ingest(imgs).box
    assert torch.equal(box, stacked)
    toks, logp = w.model.generate(box, 12, return_logp=True)
    rt, rl = w.model.generate(stacked, 12, return_logp=True)
    assert torch.equal(toks, rt) and torch.equal(logp, rl)
    trg = torch.cat((torch.full((3, 1), w.model.bos_token, dtype=torch.int64, device="cuda"), rt), 1)
    assert torch.equal(w.model.score(box, trg).logp, w.model.score(stacked, trg).logp)


# ---- 4. the opt-in hybrid front end ------------------------------------------------------------------------------------------------------
def test_hybrid_front_end_by_either_ingest(tmp_path):
    w = _wrapper(tmp_path, in_channels=1, max_batch=3, img_size=[160, 1008], embed="hybrid")
    assert w.dims.embed == "hybrid" and w.model.ragged_hybrid
    imgs = _pil_list()[:3]
    enc_h, n_h = w.model.encoder.forward_ragged([w._tensor(im).cuda() for im in imgs])
    enc_d, n_d = w.model.encoder.forward_ragged(w.model.ingest(imgs))
    assert torch.equal(n_h, n_d) and torch.equal(enc_h, enc_d)


# ---- 5. refusals reach Python ------------------------------------------------------------------------------------------------------------
def test_refusals_reach_python(wrappers):
    from texocr_amd import ops
    w = wrappers[1]
    m, eng = w.model, w.model._engine
    good = np.zeros((20, 40, 3), np.uint8)
    with pytest.raises(ValueError, match=r"ingest: image 1 has ch = 2; the channel count must be 1 \(L\), 3 \(RGB\) or 4 \(RGBA\)"):
        m.ingest([good, np.zeros((4, 4, 2), np.uint8)])
    with pytest.raises(ValueError, match=r"ingest: no images \(B must be >= 1\)"):
        m.ingest([])
    with pytest.raises(ValueError, match="pack_u8: image 1 must be uint8, got float32"):
        m.ingest([good, np.zeros((4, 4, 3), np.float32)])
    staged, dev, src, shapes = ops.plan_u8([good, np.zeros((17, 33), np.uint8)])
    bufs = [staged.cuda()]
    for hc, wc in ((16, 48), (32, 32)):                            # a container that is too small
        with pytest.raises(ValueError, match="ingest: image [01] is .* it does not fit the container's %dx%d" % (hc, wc)):
            torch.ops.texocr.ingest_u8(bufs, src, shapes, eng.id, 1, hc, wc)
    with pytest.raises(ValueError, match="multiple of 4"):
        torch.ops.texocr.ingest_u8(bufs, src, shapes, eng.id, 1, 32, 50)
    with pytest.raises(ValueError, match="reach beyond"):          # the binding's own: the bytes named must lie inside the buffer
        torch.ops.texocr.ingest_u8([bufs[0][:100]], src, shapes, eng.id, 1, 32, 48)
    with pytest.raises(ValueError, match="batch exceeds engine max_batch"):
        m.ingest([good] * (eng.max_batch + 1))
    # ... and the engine is as it was
    box, sizes = torch.ops.texocr.ingest_u8(bufs, src, shapes, eng.id, 1, 32, 48)
    assert sizes.tolist() == [[32, 48], [32, 48]] and torch.equal(box[0, 0, :20, :40], torch.ones((20, 40), device="cuda"))


# ---- the torch-free route --------------------------------------------------------------------------------------------------------------
def test_torch_free_c_program_from_bytes_to_tokens(tmp_path):
    """examples/ingest_tiny.c: plain C + the HIP runtime API: txo_ingest_box + txo_ingest_u8 + txo_generate_ragged; it compares the container
    with the same preprocessing done in C on the host, and the tokens with those of the host-made container"""
    import subprocess
    import sys
    from texocr_amd import build as b
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = b.build_example(verbose=False, name="ingest_tiny")
    blob = str(tmp_path / "tiny.bin")
    subprocess.run([sys.executable, os.path.join(root, "examples", "make_tiny_blob.py"), blob], check=True, capture_output=True)
    r = subprocess.run([exe, blob], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "equals the host preprocessing bit for bit" in r.stdout and "equal the host container's" in r.stdout
    assert "ch = 2 -> -1 (ingest: image 1 has ch = 2" in r.stdout
