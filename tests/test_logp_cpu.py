"""No-GPU checks of generate()'s per-token log-probabilities (include/texocr.h: txo_generate_logp / txo_generate_from_enc_logp /
txo_generate_ragged_logp): header / binding / export consistency of the three symbols, the argument refusals that need no device,
the operators' fake implementations, and the facade's refusal of beam search."""
import ctypes as C
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGP = ("txo_generate_logp", "txo_generate_from_enc_logp", "txo_generate_ragged_logp")
SIBLING = {"txo_generate_logp": "txo_generate", "txo_generate_from_enc_logp": "txo_generate_from_enc",
           "txo_generate_ragged_logp": "txo_generate_ragged"}


@pytest.fixture(scope="module")
def lib():
    from texocr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def _decl(hdr, name):
    return re.search(r"^int " + name + r"\((.*?)\);", hdr, re.M | re.S).group(1)


def test_logp_symbols_declared_bound_and_exported(lib):
    from texocr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "texocr.h")).read()
    for name in LOGP:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        args = [a.strip() for a in _decl(hdr, name).split(",")]
        assert len(args) == len(_lib.SYMBOLS[name][1]), name
        # the sibling's signature plus ONE argument, float* logp_out_dev, in front of the stream
        base = [a.strip() for a in _decl(hdr, SIBLING[name]).split(",")]
        assert len(args) == len(base) + 1 and len(_lib.SYMBOLS[name][1]) == len(_lib.SYMBOLS[SIBLING[name]][1]) + 1, name
        assert args[-2] == "float* logp_out_dev" and args[-1] == "void* stream", args[-2:]
        assert [re.sub(r"\s+", " ", a) for a in args[:-2]] == [re.sub(r"\s+", " ", a) for a in base[:-1]], name


def test_logp_entry_points_refuse_null_arguments_without_gpu(lib):
    from texocr_amd import _lib
    sizes = (C.c_int32 * 2)(16, 16)
    n = C.c_int32(0)
    buf = (C.c_float * 8)()
    tok = (C.c_int64 * 8)()
    p = lambda a: C.cast(a, C.c_void_p)
    fake = C.c_void_p(8)                # a non-null handle is not dereferenced before the pointers are checked
    for e in (None, fake):
        # null logp_out with everything else in place
        assert lib.txo_generate_logp(e, p(buf), 1, 3, 16, 16, 4, -1, p(tok), C.byref(n), None, None, None) == _lib.TXO_E_INVALID
        assert "null" in lib.txo_last_error().decode()
        assert lib.txo_generate_from_enc_logp(e, p(buf), 1, 2, 4, -1, p(tok), C.byref(n), None, None, None) == _lib.TXO_E_INVALID
        assert lib.txo_generate_ragged_logp(e, p(buf), 1, 3, 16, 16, sizes, 4, -1, p(tok), C.byref(n), None, None) == _lib.TXO_E_INVALID
        # null tokens_out / input
        assert lib.txo_generate_logp(e, p(buf), 1, 3, 16, 16, 4, -1, None, C.byref(n), None, p(buf), None) == _lib.TXO_E_INVALID
        assert lib.txo_generate_logp(e, None, 1, 3, 16, 16, 4, -1, p(tok), C.byref(n), None, p(buf), None) == _lib.TXO_E_INVALID
        assert lib.txo_generate_from_enc_logp(e, None, 1, 2, 4, -1, p(tok), C.byref(n), None, p(buf), None) == _lib.TXO_E_INVALID
        assert lib.txo_generate_ragged_logp(e, p(buf), 1, 3, 16, 16, None, 4, -1, p(tok), C.byref(n), p(buf), None) == _lib.TXO_E_INVALID
    assert lib.txo_generate_logp(None, p(buf), 1, 3, 16, 16, 4, -1, p(tok), C.byref(n), None, p(buf), None) == _lib.TXO_E_INVALID   # null engine
    with pytest.raises(ValueError):
        _lib.check(lib.txo_generate_logp(None, None, 1, 3, 16, 16, 4, -1, None, None, None, None, None))


def test_logp_ops_registered_with_fake_impls():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from texocr_amd import ops
    from texocr_amd.config import Dims
    d = Dims(canvas=672)

    class Stub:
        dims, device = d, 0
    stub = Stub()
    eid = ops.register_engine(stub)
    try:
        for name in ("generate_logp", "generate_from_enc_logp", "generate_ragged_logp"):
            assert hasattr(torch.ops.texocr, name), name
        with FakeTensorMode():
            img = torch.empty((4, 3, 224, 672))
            for want_logits in (False, True):
                toks, n, logp, logits = torch.ops.texocr.generate_logp(img, eid, 20, -1, want_logits)
                assert toks.shape == (4, 20) and toks.dtype == torch.int64
                assert n.shape == (1,) and n.dtype == torch.int64 and n.device.type == "cpu"
                assert logp.shape == (4, 20) and logp.dtype == torch.float32
                assert logits.shape == (4 if want_logits else 0, 20, d.vocab) and logits.dtype == torch.float32
            toks, n, logp, logits = torch.ops.texocr.generate_from_enc_logp(torch.empty((3, 589, 256)), eid, 7, 997, False)
            assert toks.shape == (3, 7) and logp.shape == (3, 7) and logp.dtype == torch.float32 and logits.shape == (0, 7, d.vocab)
            out = torch.ops.texocr.generate_ragged_logp(img, torch.tensor([[224, 672]] * 4, dtype=torch.int32), eid, 9, -1)
            assert len(out) == 3
            assert out[0].shape == (4, 9) and out[0].dtype == torch.int64 and out[1].shape == (1,)
            assert out[2].shape == (4, 9) and out[2].dtype == torch.float32
        # real calls on CPU tensors are refused before the engine is touched
        with pytest.raises(ValueError, match="CUDA/HIP tensor"):
            ops.generate_logp(torch.zeros(1, 3, 16, 16), eid, 4, -1, False)
        with pytest.raises(ValueError, match=r"\(B, C, Hc, Wc\)"):
            ops.generate_ragged_logp(torch.zeros(3, 16, 16), torch.tensor([[16, 16]], dtype=torch.int32), eid, 4, -1)
    finally:
        ops.unregister_engine(eid)


def test_return_logp_with_beam_search_is_refused():
    """checked before anything touches the engine: a stand-in for the model is enough"""
    from texocr_amd.model import OCRModel
    stub = types.SimpleNamespace()
    with pytest.raises(ValueError, match="beam search"):
        OCRModel.generate(stub, torch.zeros(1, 3, 16, 16), 4, beam=2, return_logp=True)
