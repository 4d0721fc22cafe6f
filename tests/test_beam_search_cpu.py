"""No-GPU checks of beam search with lengths and per-token log-probabilities (include/texocr.h: txo_beam_out, txo_beam_search,
txo_beam_search_ragged): header / binding / export consistency, the operators' fake implementations, the facade's argument refusals
against a stub engine, the wrapper's chunk arithmetic, and a float64 restatement of the length and ranking rule of beam_finish_kernel
(csrc/step.h) on hand-made cases."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("txo_beam_search", "txo_beam_search_ragged")


@pytest.fixture(scope="module")
def lib():
    from texocr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_entry_points_declared_bound_and_exported(lib):
    from texocr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "texocr.h")).read()
    for name in ENTRY:
        decl = re.search(r"^int " + name + r"\((.*?)\);", hdr, re.M | re.S)
        assert decl, name
        args = [re.sub(r"\s+", " ", a.strip()) for a in decl.group(1).split(",")]
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert len(args) == len(_lib.SYMBOLS[name][1]), (name, args)
        assert args[-3:] == ["const txo_beam_out* out", "int32_t* n_steps_out", "void* stream"], args[-3:]
    # the ragged call is the fixed-shape one with the sizes behind the container
    fixed, ragged = (len(_lib.SYMBOLS[n][1]) for n in ENTRY)
    assert ragged == fixed + 1
    # txo_beam_out: the header's fields, in order, are the binding's
    body = re.search(r"typedef struct \{(.*?)\} txo_beam_out;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(int64_t\*|float\*|int32_t\*|float)\s+(\w+);", body, re.M)
    assert [f[1] for f in fields] == [f[0] for f in _lib.TxoBeamOut._fields_] == ["tokens", "scores", "logp", "lengths", "length_alpha"]
    assert [f[0] for f in fields] == ["int64_t*", "float*", "float*", "int32_t*", "float"]
    assert C.sizeof(_lib.TxoBeamOut) == 4 * C.sizeof(C.c_void_p) + 8


def test_entry_points_refuse_null_arguments_without_gpu(lib):
    from texocr_amd import _lib
    sizes = (C.c_int32 * 2)(16, 16)
    n = C.c_int32(0)
    buf = (C.c_float * 8)()
    out = _lib.TxoBeamOut(None, None, None, None, 0.0)
    p = lambda a: C.cast(a, C.c_void_p)
    assert lib.txo_beam_search(None, p(buf), 1, 3, 16, 16, 2, 4, -1, C.byref(out), C.byref(n), None) == _lib.TXO_E_INVALID
    assert "null" in lib.txo_last_error().decode()
    fake = C.c_void_p(8)                # a non-null handle is not dereferenced before the pointers are checked
    assert lib.txo_beam_search(fake, None, 1, 3, 16, 16, 2, 4, -1, C.byref(out), C.byref(n), None) == _lib.TXO_E_INVALID
    assert lib.txo_beam_search_ragged(fake, None, 1, 3, 16, 16, sizes, 2, 4, -1, C.byref(out), C.byref(n), None) == _lib.TXO_E_INVALID
    assert lib.txo_beam_search_ragged(fake, p(buf), 1, 3, 16, 16, None, 2, 4, -1, C.byref(out), C.byref(n), None) == _lib.TXO_E_INVALID


def test_ops_registered_with_fake_impls():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from texocr_amd import ops
    from texocr_amd.config import Dims

    class Stub:
        dims, device = Dims(canvas=672), 0
    stub = Stub()
    eid = ops.register_engine(stub)
    try:
        with FakeTensorMode():
            img = torch.empty((4, 3, 224, 672))
            sizes = torch.tensor([[224, 672]] * 4, dtype=torch.int32)
            for want_logp in (False, True):
                for out in (torch.ops.texocr.beam_search(img, eid, 5, 20, 997, want_logp, 0.6),
                            torch.ops.texocr.beam_search_ragged(img, sizes, eid, 5, 20, 997, want_logp, 0.6)):
                    toks, scores, lengths, logp, n = out
                    assert toks.shape == (20, 20) and toks.dtype == torch.int64
                    assert scores.shape == (20,) and scores.dtype == torch.float32
                    assert lengths.shape == (20,) and lengths.dtype == torch.int32
                    assert logp.shape == (20 if want_logp else 0, 20) and logp.dtype == torch.float32
                    assert n.shape == (1,) and n.dtype == torch.int64 and n.device.type == "cpu"
        # real calls on CPU tensors are refused before the engine is touched: the shared op checks
        with pytest.raises(ValueError, match="CUDA/HIP tensor"):
            ops.beam_search(torch.zeros(1, 3, 16, 16), eid, 2, 4, -1, False, 0.0)
        with pytest.raises(ValueError, match=r"\(B, C, Hc, Wc\)"):
            ops.beam_search_ragged(torch.zeros(3, 16, 16), torch.tensor([[16, 16]], dtype=torch.int32), eid, 2, 4, -1, False, 0.0)
    finally:
        ops.unregister_engine(eid)


def _stub_model(max_len=32, max_batch=10):
    """a stand-in for OCRModel whose engine raises if it is reached"""
    def boom(*a, **k):
        raise AssertionError("the engine was called")
    eng = types.SimpleNamespace(max_batch=max_batch, beam_search=boom)
    return types.SimpleNamespace(decoder=types.SimpleNamespace(max_len=max_len), _engine=eng, eos_token=3)


@pytest.mark.parametrize("kw,frag", [
    (dict(beams=0), "beams in"), (dict(beams=9), "beams in"), (dict(beams=2.5), "beams in"), (dict(beams=True), "beams in"),
    (dict(max_len=0), "max_len >= 1"), (dict(max_len=33), "max_len <= decoder.max_len"), (dict(length_alpha=-0.1), "length_alpha"),
    (dict(length_alpha=float("nan")), "length_alpha"), (dict(length_alpha=float("inf")), "length_alpha"), (dict(length_alpha="1"), "length_alpha"),
    (dict(beams=6), "images * beams"),
])
def test_facade_refuses_before_any_engine_call(kw, frag):
    from texocr_amd.model import OCRModel
    args = dict(beams=2, max_len=8, length_alpha=0.0)
    args.update(kw)
    for src in (torch.zeros(2, 3, 16, 16), [torch.zeros(3, 16, 16), torch.zeros(3, 32, 16)]):
        with pytest.raises(ValueError, match="beam search") as err:
            OCRModel.beam_search(_stub_model(), src, args["beams"], args["max_len"], length_alpha=args["length_alpha"])
        assert frag in str(err.value), err.value
    for src in (torch.zeros(3, 16, 16), "picture", []):
        with pytest.raises(ValueError, match="beam search"):
            OCRModel.beam_search(_stub_model(), src, 2, 8)
    with pytest.raises(ValueError, match="1024"):
        OCRModel.beam_search(_stub_model(max_len=1025), torch.zeros(1, 3, 16, 16), 2, 8)


def test_wrapper_chunk_arithmetic():
    from texocr_amd.wrapper import beam_chunk
    assert [beam_chunk(mb, k) for mb, k in ((5, 5), (9, 5), (10, 5), (64, 5), (7, 3), (8, 8), (3, 1))] == [1, 1, 2, 12, 2, 1, 3]
    # chunks of beam_chunk images cover a list once, in order, and never ask for more than max_batch rows
    for mb, k, n in ((7, 3, 4), (9, 3, 4), (64, 5, 128), (8, 8, 3)):
        step = beam_chunk(mb, k)
        chunks = [list(range(n))[c0:c0 + step] for c0 in range(0, n, step)]
        assert sum(chunks, []) == list(range(n)) and all(len(c) * k <= mb for c in chunks)
    for mb, k in ((2, 3), (4, 5), (0, 1)):
        with pytest.raises(ValueError, match="max_batch"):
            beam_chunk(mb, k)
    for k in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="beams"):
            beam_chunk(64, k)


# ---- the length and ranking rule, restated on the host in float64 ---------------------------------------------------------------------
def finish64(tokens, scores, eos, alpha):
    """tokens (k, n) in the search's order, scores (k,) -> (lengths, order): length = index of the first eos + 1, or n without one (or
    eos None); order = the beams best first -- alpha == 0: as they stand; alpha > 0: descending score / length ** alpha, ties in the
    search's order (a stable sort)"""
    tokens, scores = np.asarray(tokens), np.asarray(scores, np.float64)
    k, n = tokens.shape
    lengths = np.full(k, n, np.int64)
    if eos is not None:
        for r in range(k):
            hit = np.nonzero(tokens[r] == eos)[0]
            if hit.size:
                lengths[r] = hit[0] + 1
    if alpha == 0:
        return lengths, np.arange(k)
    return lengths, np.argsort(-(scores / lengths.astype(np.float64) ** alpha), kind="stable")


def test_length_and_ranking_rule_on_hand_made_cases():
    E = 9
    toks = [[1, 2, E, E, E, E],          # length 3
            [1, 2, 3, 4, 5, 6],          # no eos: 6
            [E, E, E, E, E, E],          # eos at position 0: 1
            [1, 2, 3, 4, E, E]]          # 5
    scores = [-3.0, -4.0, -2.5, -3.5]
    lengths, order = finish64(toks, scores, E, 0.0)
    assert lengths.tolist() == [3, 6, 1, 5] and order.tolist() == [0, 1, 2, 3]
    # alpha = 1: per-token averages -1, -2/3, -2.5, -0.7 -> the long beams first
    assert finish64(toks, scores, E, 1.0)[1].tolist() == [1, 3, 0, 2]
    # alpha = 0.5: -3/sqrt(3) = -1.732, -4/sqrt(6) = -1.633, -2.5, -3.5/sqrt(5) = -1.565
    assert finish64(toks, scores, E, 0.5)[1].tolist() == [3, 1, 0, 2]
    # no eos (or eos None): every length is n, the order is the search's whatever alpha is
    assert finish64(toks, scores, None, 1.0)[0].tolist() == [6, 6, 6, 6]
    assert finish64(toks, sorted(scores, reverse=True), None, 1.0)[1].tolist() == [0, 1, 2, 3]
    # ties keep the search's order: -2/2 == -3/3 == -1, and two bit-equal beams
    tie = [[1, E, E], [1, 2, E], [1, E, E]]
    lengths, order = finish64(tie, [-2.0, -3.0, -2.0], E, 1.0)
    assert lengths.tolist() == [2, 3, 2] and order.tolist() == [0, 1, 2]
    assert finish64(tie, [-2.0, -2.9, -2.0], E, 1.0)[1].tolist() == [1, 0, 2]
    # dead beams (score -inf, fewer candidates than beams) stay last, in order
    assert finish64([[1, 2], [3, 4], [5, 6]], [-1.0, -np.inf, -np.inf], E, 0.7)[1].tolist() == [0, 1, 2]
