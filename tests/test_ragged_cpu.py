"""No-GPU checks of the ragged-batch surface (include/texocr.h: txo_encode_ragged / txo_decode_begin_ragged / txo_generate_ragged):
the container layout pack_ragged builds and its errors, header / export / query-code consistency of the new symbols, and the argument
refusals that need no device."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = ("txo_encode_ragged", "txo_decode_begin_ragged", "txo_generate_ragged")


@pytest.fixture(scope="module")
def lib():
    from texocr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_pack_ragged_layout():
    from texocr_amd.ops import pack_ragged, ragged_tokens
    gen = torch.Generator().manual_seed(0)
    images = [torch.rand((3, h, w), generator=gen) + 0.5 for h, w in ((32, 48), (16, 128), (64, 16))]
    box, sizes = pack_ragged(images)
    assert box.shape == (3, 3, 64, 128) and box.dtype == torch.float32 and box.is_contiguous()
    assert sizes.dtype == torch.int32 and not sizes.is_cuda and sizes.tolist() == [[32, 48], [16, 128], [64, 16]]
    assert ragged_tokens(sizes).tolist() == [7, 9, 5] and ragged_tokens(sizes).dtype == torch.int32
    for b, im in enumerate(images):
        h, w = im.shape[1:]
        assert torch.equal(box[b, :, :h, :w], im)                      # top-left corner
        rest = box[b].clone()
        rest[:, :h, :w] = 0
        assert float(rest.abs().max()) == 0.0                          # everything else is zero
    one, s1 = pack_ragged([images[0]])
    assert one.shape == (1, 3, 32, 48) and torch.equal(one[0], images[0]) and s1.tolist() == [[32, 48]]


@pytest.mark.parametrize("images,frag", [
    ([], "no images"),
    ([torch.zeros(3, 20, 32)], "multiples of 16"),
    ([torch.zeros(3, 16, 0)], "multiples of 16"),
    ([torch.zeros(3, 16, 16), torch.zeros(1, 16, 16)], r"must be \(3, H, W\)"),
    ([torch.zeros(3, 16, 16), torch.zeros(16, 16)], r"must be \(3, H, W\)"),
    ([torch.zeros(3, 16, 16, dtype=torch.float64)], "float32"),
])
def test_pack_ragged_errors(images, frag):
    from texocr_amd.ops import pack_ragged
    with pytest.raises(ValueError, match=frag):
        pack_ragged(images)


def test_ragged_symbols_declared_bound_and_exported(lib):
    from texocr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "texocr.h")).read()
    for name in RAGGED:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    # argument counts of the binding follow the header's declarations
    for name in RAGGED:
        decl = re.search(r"^int " + name + r"\((.*?)\);", hdr, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[name][1]), name
    assert re.search(r"^#define\s+TXO_Q_LAST_RAGGED\s+7\b", hdr, re.M) and _lib.Q_LAST_RAGGED == 7


def test_ragged_ops_are_registered():
    import texocr_amd.ops  # noqa: F401
    for name in ("encode_ragged", "decode_begin_ragged", "generate_ragged"):
        assert hasattr(torch.ops.texocr, name), name


def test_ragged_null_arguments_need_no_device(lib):
    from texocr_amd import _lib
    sizes = (C.c_int32 * 2)(16, 16)
    n = C.c_int32(0)
    assert lib.txo_encode_ragged(None, None, 1, 3, 16, 16, sizes, None, C.byref(n), None) == _lib.TXO_E_INVALID
    assert lib.txo_decode_begin_ragged(None, None, 1, 2, sizes, None) == _lib.TXO_E_INVALID
    assert lib.txo_generate_ragged(None, None, 1, 3, 16, 16, sizes, 4, -1, None, C.byref(n), None) == _lib.TXO_E_INVALID
    assert "null" in lib.txo_last_error().decode()


def test_ragged_ops_refuse_cpu_tensors_and_bad_sizes():
    """the operators check their tensors before the engine is touched (no GPU: the engine object is a stand-in with dims only)"""
    from texocr_amd import ops
    from texocr_amd.config import Dims

    class Stub:
        dims = Dims(canvas=64)
        device = 0
    stub = Stub()
    i = ops.register_engine(stub)
    try:
        with pytest.raises(ValueError, match="CUDA/HIP tensor"):
            ops.encode_ragged(torch.zeros(1, 3, 16, 16), torch.tensor([[16, 16]], dtype=torch.int32), i)
        with pytest.raises(ValueError, match=r"\(B, C, Hc, Wc\)"):
            ops.generate_ragged(torch.zeros(3, 16, 16), torch.tensor([[16, 16]], dtype=torch.int32), i, 4, -1)
    finally:
        ops.unregister_engine(i)
