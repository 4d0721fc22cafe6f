"""No-GPU checks of the ragged multi-position forward's host side (tests/test_gpu_ragged_forward.py has the GPU tests): the new symbol and
operator, the facades' argument errors that are raised before the engine is touched, the grid / crop arithmetic of alignment_ragged on
synthetic head-mean maps, and what TeXOCRWrapper.batch(return_align=True) hands to align_ragged."""
import ctypes as C
import os
import re
import types

import pytest
import torch

from texocr_amd.config import Dims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = Dims(canvas=64, in_channels=3, embed_dim=64, enc_heads=2, enc_layers=1, dec_heads=2, dec_layers=3, vocab=64, max_len=24, bos=62, eos=61,
         pad=63)


def test_score_ragged_declared_bound_exported_and_registered():
    from texocr_amd import build, _lib, ops  # noqa: F401  (importing ops registers the operators)
    build.build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "texocr.h")).read()
    decl = re.search(r"^int txo_score_ragged\((.*?)\);", hdr, re.M | re.S).group(1)
    assert len(decl.split(",")) == len(_lib.SYMBOLS["txo_score_ragged"][1]) == 14 and hasattr(lib, "txo_score_ragged")
    tok, buf, sizes = (C.c_int64 * 8)(), (C.c_float * 8)(), (C.c_int32 * 2)(16, 16)
    p = lambda a: C.cast(a, C.c_void_p)
    assert lib.txo_score_ragged(None, p(buf), 1, 3, 16, 16, sizes, p(tok), None, 4, None, None, None, None) == _lib.TXO_E_INVALID
    assert "null" in lib.txo_last_error().decode()
    assert lib.txo_set_ragged_forward(None, 1) == _lib.TXO_E_INVALID and "null" in lib.txo_last_error().decode()
    assert hasattr(torch.ops.texocr, "score_ragged")
    assert "no ragged form" not in hdr and "txo_decode_begin_ragged" in hdr


def test_score_ragged_op_fake_shapes_and_cpu_refusal():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from texocr_amd import ops

    class Stub:
        dims, device, session = D, 0, None
    stub = Stub()
    eid = ops.register_engine(stub)
    try:
        with FakeTensorMode():
            out = torch.ops.texocr.score_ragged(torch.empty((3, 3, 32, 48)), torch.tensor([[32, 48]] * 3, dtype=torch.int32),
                                                torch.empty((3, 9), dtype=torch.int64), None, eid)
            assert [tuple(o.shape) for o in out] == [(3, 8)] * 3 and out[1].dtype == torch.int64
        with pytest.raises(ValueError, match="no CPU path"):
            ops.score_ragged(torch.zeros((1, 3, 16, 16)), torch.tensor([[16, 16]], dtype=torch.int32), torch.zeros((1, 4), dtype=torch.int64), None, eid)
        # the session record names its own key count where the source tensor does not: the slot stride behind score_ragged
        box = torch.empty((2, 3, 64, 64))
        assert ops._session_keys(stub, ops.Session(2, box)) == 17
        assert ops._session_keys(stub, ops.Session(2, box, keys=5)) == 5
        assert ops._session_keys(stub, ops.Session(2, torch.empty((2, 9, 64)))) == 9
    finally:
        ops.unregister_engine(eid)


def _decoder():
    from texocr_amd import model
    touched = []
    eng = types.SimpleNamespace(dims=D, decode_begin=lambda *a: touched.append("begin"), decode_begin_ragged=lambda *a: touched.append("begin_ragged"))
    dec = types.SimpleNamespace(_engine=eng, max_len=D.max_len)
    return model, dec, touched


@pytest.mark.parametrize("n_tokens,frag", [(torch.tensor([5, 5], dtype=torch.int32), "one entry per row"),
                                           (torch.tensor([[5, 5, 5]], dtype=torch.int32), "one entry per row"),
                                           (torch.tensor([5, 0, 5], dtype=torch.int32), r"in \[1, 7\]"),
                                           (torch.tensor([5, 8, 5], dtype=torch.int32), r"in \[1, 7\]")])
def test_n_tokens_errors_come_before_the_engine(n_tokens, frag):
    model, dec, touched = _decoder()
    enc, x = torch.zeros((3, 7, 64)), torch.zeros((3, 5), dtype=torch.int64)
    for call in (lambda: model.Transformer.forward(dec, x, enc=enc, n_tokens=n_tokens),
                 lambda: model.AutoRegressiveDecoder.score(dec, x, enc=enc, n_tokens=n_tokens),
                 lambda: model.AutoRegressiveDecoder.align(dec, x, enc=enc, n_tokens=n_tokens)):
        with pytest.raises(ValueError, match=frag):
            call()
    assert touched == []


def test_facade_argument_errors(monkeypatch):
    model, dec, touched = _decoder()
    enc, x = torch.zeros((3, 7, 64)), torch.zeros((3, 5), dtype=torch.int64)
    n = torch.tensor([7, 2, 5], dtype=torch.int32)
    with pytest.raises(ValueError, match="one .rows, cols. per image"):
        model.AutoRegressiveDecoder.align(dec, x, enc=enc, n_tokens=n, grids=[(2, 3)])
    with pytest.raises(ValueError, match="pass n_tokens"):
        model.AutoRegressiveDecoder.align(dec, x, enc=enc, grids=[(2, 3)] * 3)
    monkeypatch.setattr(model, "_check_x", lambda *a: None)                          # (it wants GPU tensors)
    long = torch.zeros((3, D.max_len + 2), dtype=torch.int64)
    for call in (lambda: model.AutoRegressiveDecoder.score(dec, long, enc=enc, n_tokens=n),
                 lambda: model.AutoRegressiveDecoder.align(dec, long, enc=enc, n_tokens=n)):
        with pytest.raises(ValueError, match="longer than decoder.max_len"):
            call()
    bad = x.clone()
    bad[1, 2] = D.vocab
    with pytest.raises(IndexError, match="outside the vocabulary"):
        model.AutoRegressiveDecoder.score(dec, bad, enc=enc, n_tokens=n)
    with pytest.raises(ValueError, match="prefix longer"):
        model.Transformer.forward(dec, torch.zeros((3, D.max_len + 1), dtype=torch.int64), enc=enc, n_tokens=n)
    assert touched == []
    # OCRModel.score_ragged / align_ragged: trg against the images
    ocr = types.SimpleNamespace(decoder=dec, trg_pad_idx=D.pad, _engine=dec._engine)
    ocr._ragged_trg = lambda *a: model.OCRModel._ragged_trg(ocr, *a)
    images = [torch.zeros((3, 16, 16)), torch.zeros((3, 32, 16))]
    for fn in (model.OCRModel.score_ragged, model.OCRModel.align_ragged):
        with pytest.raises(ValueError, match="one row per image"):
            fn(ocr, images, torch.zeros((3, 5), dtype=torch.int64))
        with pytest.raises(ValueError, match="at least two columns"):
            fn(ocr, images, torch.zeros((2, 1), dtype=torch.int64))
        with pytest.raises(ValueError, match="longer than decoder.max_len"):
            fn(ocr, images, torch.zeros((2, D.max_len + 2), dtype=torch.int64))
        with pytest.raises(ValueError, match="shape of trg"):
            fn(ocr, images, torch.zeros((2, 5), dtype=torch.int64), torch.ones((2, 4), dtype=torch.bool))
    with pytest.raises(IndexError, match="outside the vocabulary"):
        model.OCRModel.score_ragged(ocr, images, torch.full((2, 5), -1, dtype=torch.int64))
    assert touched == []


def test_alignment_ragged_crops_to_the_images_own_grid():
    from texocr_amd.model import alignment, alignment_ragged
    grids = [(2, 3), (1, 1), (4, 2)]
    n = [1 + h * w for h, w in grids]                                                # 7, 2, 9
    Ns, Ld, t = max(n), 3, 5
    g = torch.Generator().manual_seed(0)
    mean = torch.zeros((Ld, 3, t, Ns))
    for b, nb in enumerate(n):
        mean[:, b, :, :nb] = torch.softmax(3 * torch.randn((Ld, t, nb), generator=g), dim=-1)
    junk = mean.clone()
    for b, nb in enumerate(n):
        junk[:, b, :, nb:] = 7.0                                                     # whatever stands behind n_b is cut off, never looked at
    for layer in (-1, 0, None):
        out = alignment_ragged(mean, n, layer, grids)
        assert len(out) == 3
        for b, (a, (h, w)) in enumerate(zip(out, grids)):
            solo = alignment(mean[:, b:b + 1, :, :n[b]].contiguous(), layer, (h, w))
            assert a.maps.shape == (1, t, h, w) and a.cls.shape == (1, t) and a.peak.shape == (1, t, 2)
            assert torch.equal(a.maps, solo.maps) and torch.equal(a.cls, solo.cls) and torch.equal(a.peak, solo.peak)
            assert float((a.maps.sum(dim=(2, 3)) + a.cls - 1).abs().max()) < 1e-6
            assert bool((a.peak[..., 0] < h).all()) and bool((a.peak[..., 1] < w).all())
        for a, j in zip(out, alignment_ragged(junk, n, layer, grids)):
            assert torch.equal(a.maps, j.maps) and torch.equal(a.peak, j.peak)
    flat = alignment_ragged(mean, torch.tensor(n, dtype=torch.int32).tolist(), -1, None)
    assert [tuple(a.maps.shape) for a in flat] == [(1, t, nb - 1) for nb in n] and flat[0].peak.shape == (1, t)
    with pytest.raises(ValueError, match="does not hold"):
        alignment_ragged(mean, n, -1, [(2, 3), (1, 1), (3, 3)])
    with pytest.raises(ValueError, match="one entry per image"):
        alignment_ragged(mean, n[:2], -1, None)


def test_wrapper_align_inputs():
    from texocr_amd.wrapper import align_inputs, cut_at_eos
    eos, bos, pad = 61, 62, 63
    rows = [[5, 6, eos, pad, pad], [7, 8, 9, 10, 11], [eos, pad, pad, pad, pad]]     # an eos in the middle, none, at once
    full = [cut_at_eos(r, eos) for r in rows]
    assert full == [[5, 6, eos], [7, 8, 9, 10, 11], [eos]]
    assert cut_at_eos([1, 2, 3], None) == [1, 2, 3]
    trg, mask = align_inputs(full, bos, pad)
    assert trg.dtype == torch.int64 and mask.dtype == torch.bool and trg.shape == mask.shape == (3, 6)
    assert trg.tolist() == [[bos, 5, 6, eos, pad, pad], [bos, 7, 8, 9, 10, 11], [bos, eos, pad, pad, pad, pad]]
    assert mask.sum(1).tolist() == [4, 6, 2] and bool((mask == (torch.arange(6)[None] < torch.tensor([4, 6, 2])[:, None])).all())
    # position p of row b (p < len(full[b])) is fed trg[b, p] and produced full[b][p]; the kept tokens are full[b][:-1]
    for b, r in enumerate(full):
        assert trg[b, 1:1 + len(r)].tolist() == r and bool(mask[b, :len(r)].all())
