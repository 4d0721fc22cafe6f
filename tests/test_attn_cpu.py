"""No-GPU checks of the decoder attention maps (include/texocr.h: txo_decode_attn): the float64 helper tests/attn_ref.py against the
reference's own maps (tests/golden/attn_*.npz), header / binding / export consistency, the operator's fake implementation, the refusals
that need no device, the Alignment arithmetic on a stand-in engine, and the room the bf16 bound of tests/test_gpu_attn.py leaves."""
import contextlib
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import attn_ref
from oracle import cpu_ref
from texocr_amd import synth
from texocr_amd.config import Dims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _fixture(name):
    meta = json.load(open(os.path.join(GOLD, name + ".json")))
    g = np.load(os.path.join(GOLD, name + ".npz"))
    d = Dims(**meta["dims"])
    sd = synth.synth_state_dict(d, meta["weight_seed"])
    img = torch.from_numpy(synth.synth_images(*meta["image_shape"], seed=meta["image_seed"]))
    enc = cpu_ref.encode(cpu_ref.to_torch_sd(sd), img)
    x, mask = torch.from_numpy(g["x"].astype(np.int64)), torch.from_numpy(g["mask"].astype(bool))
    return d, sd, enc, x, mask, [torch.from_numpy(g[f"map{i}"]) for i in range(2 * d.dec_layers)]


@pytest.mark.parametrize("name", ["attn_tiny", "attn_pad"])
def test_float64_helper_reproduces_the_reference_maps(name):
    d, sd, enc, x, mask, ref = _fixture(name)
    assert bool(mask.all()) == (name == "attn_tiny")
    _, maps = attn_ref.decoder_attn(attn_ref.sd64(sd), x, enc, mask)
    assert len(maps) == len(ref) == 2 * d.dec_layers
    t = x.shape[1]
    future = torch.triu(torch.ones((t, t), dtype=torch.bool), diagonal=1)
    for i, (got, want) in enumerate(zip(maps, ref)):
        assert got.shape == want.shape == (x.shape[0], d.dec_heads, t, t if i % 2 == 0 else enc.shape[1]), i
        err = (got - want.double()).abs().permute(1, 3, 0, 2)[..., mask]
        assert float(err.max()) < 1e-6, (i, float(err.max()))
        for m in (got, want.double()):
            rows = m.sum(-1).permute(1, 0, 2)[:, mask]
            assert float((rows - 1).abs().max()) < 1e-6
            if i % 2 == 0:                                                 # (a padded query's row is uniform over all keys)
                assert bool((m.permute(0, 2, 3, 1)[future[None] & mask[:, :, None]] == 0).all()), "causal zeros are exact"


def test_symbol_declared_bound_and_exported_and_null_refusals():
    from texocr_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "texocr.h")).read()
    decl = re.search(r"^int txo_decode_attn\((.*?)\);", hdr, re.M | re.S).group(1)
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")]
    assert len(args) == len(_lib.SYMBOLS["txo_decode_attn"][1]) == 8 and hasattr(lib, "txo_decode_attn")
    assert args[3:] == ["float* logits_out_dev", "float* self_attn_out_dev", "float* cross_attn_out_dev", "float* cross_mean_out_dev", "void* stream"]
    tok, buf = (C.c_int64 * 8)(), (C.c_float * 8)()
    p = lambda a: C.cast(a, C.c_void_p)
    assert lib.txo_decode_attn(None, p(tok), 2, None, p(buf), None, None, None) == _lib.TXO_E_INVALID     # null engine
    assert "null" in lib.txo_last_error().decode()


def test_op_registered_with_fake_impl():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from texocr_amd import ops
    d = Dims(canvas=672)
    assert hasattr(torch.ops.texocr, "decode_attn")

    class Stub:
        dims, device, session = d, 0, None
    stub = Stub()
    eid = ops.register_engine(stub)
    try:
        with FakeTensorMode():
            x = torch.empty((4, 33), dtype=torch.int64)
            for src, N in ((torch.empty((4, 589, 256)), 589), (torch.empty((4, 3, 224, 448)), 1 + 14 * 28)):
                stub.session = ops.Session(4, src)
                for wl, ws, wc, wm in ((True, True, True, True), (False, True, False, False), (False, False, True, False), (False, False, False, True)):
                    lg, sp, cp, mean = torch.ops.texocr.decode_attn(x, eid, wl, ws, wc, wm)
                    assert lg.shape == (4 if wl else 0, 33, d.vocab)
                    assert sp.shape == (d.dec_layers if ws else 0, 4, d.dec_heads, 33, 33)
                    assert cp.shape == (d.dec_layers if wc else 0, 4, d.dec_heads, 33, N)
                    assert mean.shape == (d.dec_layers if wm else 0, 4, 33, N)
                    assert all(o.dtype == torch.float32 for o in (lg, sp, cp, mean))
                assert stub.session.rows == 4 and stub.session.src is src and stub.session.mask is None      # the record is left alone
        stub.session = None
        with pytest.raises(RuntimeError, match="needs a session"):
            ops.decode_attn(torch.zeros((4, 3), dtype=torch.int64), eid, True, True, True, False)
        stub.session = ops.Session(4, torch.empty((4, 7, 256)))
        with pytest.raises(ValueError, match="int64 GPU tensor"):                       # a real call on CPU tensors is refused
            ops.decode_attn(torch.zeros((4, 3), dtype=torch.int64), eid, True, True, True, False)
    finally:
        ops.unregister_engine(eid)


def test_return_embeddings_and_unknown_keywords_stay_refused():
    from texocr_amd.model import Transformer
    stub = types.SimpleNamespace()
    x = torch.zeros((1, 2), dtype=torch.int64)
    for kw in ({"return_embeddings": True}, {"return_attn": True, "return_embeddings": False}, {"return_hidden": True}):
        with pytest.raises(ValueError, match="unsupported arguments for the inference path"):
            Transformer.forward(stub, x, enc=torch.zeros((1, 2, 64)), **kw)


class _StubEngine:
    """decode_attn of a stand-in engine: random head-mean maps whose rows sum to 1"""

    def __init__(self, d, N):
        self.dims, self.N, self.calls = d, N, []

    def decode_begin(self, enc):
        self.calls.append("begin")

    @contextlib.contextmanager
    def key_mask(self, mask):
        self.calls.append(("mask", None if mask is None else tuple(mask.shape)))
        yield mask is not None

    def decode_attn(self, x, want_logits=True, want_self=True, want_cross=True, want_mean=False):
        assert (want_logits, want_self, want_cross, want_mean) == (False, False, False, True), "align asks for the head mean only"
        g = torch.Generator().manual_seed(0)
        self.mean = torch.softmax(3 * torch.randn((self.dims.dec_layers, x.shape[0], x.shape[1], self.N), generator=g), dim=-1)
        return None, None, None, self.mean


def test_alignment_on_a_stand_in_engine(monkeypatch):
    from texocr_amd import model
    monkeypatch.setattr(model, "_check_x", lambda *a: None)                          # (it wants GPU tensors)
    d = Dims(canvas=64, in_channels=3, embed_dim=64, enc_heads=2, enc_layers=1, dec_heads=2, dec_layers=3, vocab=64, max_len=24, bos=62,
             eos=61, pad=63)
    eng = _StubEngine(d, 1 + 2 * 3)
    dec = types.SimpleNamespace(_engine=eng, max_len=d.max_len)
    dec.align = lambda *a, **k: model.AutoRegressiveDecoder.align(dec, *a, **k)
    ocr = types.SimpleNamespace(decoder=dec, trg_pad_idx=d.pad, encoder=lambda src: torch.zeros((src.shape[0], eng.N, d.embed_dim)))
    ocr.encoder.patch_size = 16
    src, trg = torch.zeros((2, 3, 32, 48)), torch.randint(0, 60, (2, 9))
    trg[1, 5:] = d.pad
    for layer in (-1, 0, 1, None):
        a = model.OCRModel.align(ocr, src, trg, layer=layer)
        want = eng.mean.mean(0) if layer is None else eng.mean[layer]
        assert isinstance(a, model.Alignment) and a._fields == ("maps", "cls", "peak")
        assert a.maps.shape == (2, 8, 2, 3) and a.cls.shape == (2, 8) and a.peak.shape == (2, 8, 2)
        assert torch.equal(a.maps.reshape(2, 8, 6), want[..., 1:]) and torch.equal(a.cls, want[..., 0])
        assert float((a.maps.sum(dim=(2, 3)) + a.cls - 1).abs().max()) < 1e-6
        assert torch.equal(a.peak[..., 0] * 3 + a.peak[..., 1], want[..., 1:].argmax(-1))
    assert ("mask", (2, 8)) in eng.calls                                               # the mask of the fed columns, as score() sets it
    flat = model.AutoRegressiveDecoder.align(dec, trg, enc=torch.zeros((2, 7, 64)))
    assert flat.maps.shape == (2, 8, 6) and flat.peak.shape == (2, 8)
    with pytest.raises(ValueError, match="layer must be"):
        model.AutoRegressiveDecoder.align(dec, trg, enc=torch.zeros((2, 7, 64)), layer=3)


def test_sharp_case_outruns_float32_exp():
    c = attn_ref.case("h1_sharp", *attn_ref.SHARP_CASE)
    assert attn_ref.future_excess(c) > 110                          # exp(-104) is the last float32 that is not 0
    assert bool(torch.isfinite(c.self64).all()) and float((c.self64.sum(-1) - 1).abs().max()) < 1e-12


def test_bf16_bound_tells_the_layers_apart():
    """the bound tests/test_gpu_attn.py asserts for a bf16 engine stays strictly below the distance between the float64 maps of any two
    layers of every case it is asserted on (from the reference arithmetic alone): maps of the wrong layer cannot pass it"""
    assert attn_ref.BF16_BOUND == 2 * attn_ref.BF16_MEASURED
    for name, (d, ws, B, N, t, seed, lengths) in attn_ref.BF16_CASES.items():
        c = attn_ref.case(name, d, ws, B, N, t, seed, lengths)
        for kind, stack in (("self", c.self64), ("cross", c.cross64), ("head mean", c.cross64.mean(dim=2, keepdim=True))):
            dist = attn_ref.layer_distance(stack, c.valid())
            assert attn_ref.BF16_BOUND < dist, (name, kind, dist)
