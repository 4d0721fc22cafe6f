"""No-GPU checks of the prompted decode (include/texocr.h: txo_generate_prefix / _from_enc / _ragged): the host restatement of its column
rule (tests/prefix_ref.py) against the reference's captured tokens and against the reference loop with an eos, the three symbols and
operators, and every refusal -- each before anything touches an engine, each naming the prefix."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import cpu_ref
from texocr_amd import synth
from texocr_amd.config import Dims

import prefix_ref
import ref64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("txo_generate_prefix", "txo_generate_prefix_from_enc", "txo_generate_prefix_ragged")


@pytest.fixture(scope="module")
def lib():
    from texocr_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def fixture64():
    meta, g = load_golden("ragged_prefix")
    d = Dims(**meta["dims"])
    sd = ref64.sd64(synth.synth_state_dict(d, meta["weight_seed"]))
    img = torch.from_numpy(synth.synth_images(*meta["image_shape"], seed=meta["image_seed"])).double()
    return meta, g, d, sd, img, torch.from_numpy(g["start"].astype(np.int64))


def test_equal_lengths_are_the_reference(fixture64):
    """with equal lengths the column rule is the reference's output[:, T:]: the fixture's tokens_unmasked, captured from the reference"""
    meta, g, d, sd, img, start = fixture64
    assert float(g["margin"].min()) >= 1e-4
    ref = prefix_ref.generate_prefix(sd, img, start, None, None, meta["max_len"], d.pad, bos=d.bos)
    assert np.array_equal(ref.tokens.numpy(), g["tokens_unmasked"])
    assert ref.t_last == start.shape[1] + meta["max_len"] - 2
    assert bool((ref.prefix_logp == 0).all())                     # m == P: nothing is forced inside the loop
    assert bool(torch.isfinite(ref.margin).all()) and bool((ref.logp < 0).all())


def test_global_break_is_the_reference_loops(fixture64):
    """equal lengths with an eos: the break position and the columns are cpu_ref.generate_recompute's with that eos, for every token that
    occurs in the continuation (and one that occurs in a prefix: finished from the start)"""
    meta, g, d, sd, img, start = fixture64
    free = torch.from_numpy(g["tokens_unmasked"].astype(np.int64))
    for eos in sorted(set(free.flatten().tolist()))[:6] + [int(start[1, 1])]:
        want = cpu_ref.generate_recompute(sd, img, d.bos, eos, meta["max_len"], start_tokens=start)
        got, reached, t_last = prefix_ref.combine(start, [start.shape[1]] * 3, free, eos, meta["max_len"], d.pad)
        assert np.array_equal(got.numpy(), want.numpy()), eos
        assert bool(reached.all()) and t_last == start.shape[1] - 1 + want.shape[1] - 1
        # stop='row': the oracle's pad rule (start tokens included in the test) and the facade's _pad_after_eos agree with the column rule
        row = prefix_ref.combine(start, [start.shape[1]] * 3, free, eos, meta["max_len"], d.pad, stop="row")[0]
        assert np.array_equal(row.numpy(), cpu_ref.pad_after_eos(torch.cat([start, want], 1), start.shape[1], eos, d.pad).numpy()), eos
        from texocr_amd.model import _pad_after_eos
        assert torch.equal(row, _pad_after_eos(want, start, eos, d.pad)), eos


def test_per_row_lengths_column_rule():
    """by hand: lengths (1, 3, 2), max_len 4, eos 9.  Row 0 picks from position 0; row 1 is forced at positions 0 and 1 and picks from 2;
    row 2's prefix holds eos.  Row 1 picks eos in its column 1 (position 3), row 0 in column 2 (position 2): break after position 3."""
    prefix = torch.tensor([[5, 0, 0], [5, 6, 7], [5, 9, 0]])
    free = torch.tensor([[1, 2, 9, 3], [4, 9, 8, 8], [1, 1, 1, 1]])
    tok, reached, t_last = prefix_ref.combine(prefix, [1, 3, 2], free, 9, 4, pad=0)
    assert t_last == 3 and tok.shape == (3, 4)
    assert tok.tolist() == [[1, 2, 9, 3], [4, 9, 0, 0], [1, 1, 1, 0]]
    assert reached.tolist() == [[True] * 4, [True, True, False, False], [True, True, True, False]]
    row = prefix_ref.combine(prefix, [1, 3, 2], free, 9, 4, pad=0, stop="row")[0]
    assert row.tolist() == [[1, 2, 9, 0], [4, 9, 0, 0], [0, 0, 0, 0]]
    # no eos: every row gets max_len columns, the loop runs to position max(len) + max_len - 2
    tok, reached, t_last = prefix_ref.combine(prefix, [1, 3, 2], free, None, 4, pad=0)
    assert t_last == 5 and bool(reached.all()) and torch.equal(tok, free)
    # a prefix that holds eos ANYWHERE in its own length counts from the start (decoder.py:115 tests the whole output), also where the loop
    # has yet to force it: both rows are finished, one position is decoded, row 1 never gets behind its prefix (pad)
    p2 = torch.tensor([[9, 0, 0], [5, 6, 9]])
    tok, _, t_last = prefix_ref.combine(p2, [1, 3], torch.tensor([[1, 1], [2, 2]]), 9, 2, pad=0)
    assert t_last == 0 and tok.tolist() == [[1], [0]]
    # ... but not behind its length
    tok, _, t_last = prefix_ref.combine(p2, [1, 2], torch.tensor([[1, 1], [2, 2]]), 9, 2, pad=0)
    assert t_last == 2 and tok.tolist() == [[1, 1], [2, 2]]


def _decl(hdr, name):
    return re.search(r"^int " + name + r"\((.*?)\);", hdr, re.M | re.S).group(1)


def test_symbols_declared_bound_and_exported(lib):
    from texocr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "texocr.h")).read()
    for name in ENTRY:
        args = [re.sub(r"\s+", " ", a.strip()) for a in _decl(hdr, name).split(",")]
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert len(args) == len(_lib.SYMBOLS[name][1]), (name, args)
        # behind the images every entry point takes the same ten arguments
        assert args[-10:] == ["const int64_t* prefix_dev", "int32_t P", "const int32_t* prefix_len_host", "int32_t max_len", "int32_t eos",
                              "int64_t* tokens_out_dev", "int32_t* n_steps_out", "float* logp_out_dev", "float* prefix_logp_out_dev", "void* stream"]
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"({len(_lib.SYMBOLS)} entry points)" in readme


def test_entry_points_refuse_null_arguments_without_gpu(lib):
    from texocr_amd import _lib
    sizes = (C.c_int32 * 2)(16, 16)
    n = C.c_int32(0)
    buf, tok = (C.c_float * 8)(), (C.c_int64 * 8)()
    p = lambda a: C.cast(a, C.c_void_p)
    fake = C.c_void_p(8)                # a non-null handle is not dereferenced before the pointers are checked
    tail = (p(tok), 2, None, 4, -1, p(tok), C.byref(n), None, None, None)
    for e in (None, fake):
        for call in (lambda *t: lib.txo_generate_prefix(e, None if e else p(buf), 1, 3, 16, 16, *t),
                     lambda *t: lib.txo_generate_prefix_from_enc(e, None if e else p(buf), 1, 2, *t),
                     lambda *t: lib.txo_generate_prefix_ragged(e, None if e else p(buf), 1, 3, 16, 16, sizes, *t)):
            assert call(*tail) == _lib.TXO_E_INVALID
            assert "prefix" in lib.txo_last_error().decode() and "null" in lib.txo_last_error().decode()
    no_prefix = (None,) + tail[1:]
    no_out = tail[:5] + (None,) + tail[6:]
    for t in (no_prefix, no_out):
        assert lib.txo_generate_prefix(fake, p(buf), 1, 3, 16, 16, *t) == _lib.TXO_E_INVALID
        assert lib.txo_generate_prefix_from_enc(fake, p(buf), 1, 2, *t) == _lib.TXO_E_INVALID
        assert lib.txo_generate_prefix_ragged(fake, p(buf), 1, 3, 16, 16, sizes, *t) == _lib.TXO_E_INVALID
    assert lib.txo_generate_prefix_ragged(fake, p(buf), 1, 3, 16, 16, None, *tail) == _lib.TXO_E_INVALID


def test_check_prefix_refusals():
    from texocr_amd.ops import check_prefix
    assert check_prefix((3, 5), None, 8, 24) == (5, 5)
    assert check_prefix((3, 5), torch.tensor([1, 5, 3], dtype=torch.int32), 20, 24, 100) == (1, 5)
    for args, frag in (
        (((3,), None, 4, 24), r"prefix must be \(B, P\)"),
        (((3, 0), None, 4, 24), r"prefix must be \(B, P\)"),
        (((3, 5), None, 0, 24), "prefix decode: max_len"),
        (((3, 5), [1, 2], 4, 24), "prefix_len must have one entry per row"),
        (((3, 5), [0, 2, 3], 4, 24), r"prefix_len must be in \[1, 5\]"),
        (((3, 5), [1, 2, 6], 4, 24), r"prefix_len must be in \[1, 5\]"),
        (((3, 5), None, 21, 24), "longest prefix .* does not slide the window"),
        (((3, 5), [1, 1, 5], 21, 24), "longest prefix"),
        (((3, 9), [8, 9, 9], 4, 24, 6), "shortest prefix .* workspace"),
    ):
        with pytest.raises(ValueError, match=frag):
            check_prefix(*args)
    assert check_prefix((3, 5), [1, 1, 4], 21, 24) == (1, 4)       # columns behind the longest length do not count


def test_ops_registered_with_fake_impls_and_shared_checks():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from texocr_amd import ops
    d = Dims(canvas=672)

    class Stub:
        dims, device = d, 0
    stub = Stub()
    eid = ops.register_engine(stub)
    try:
        with FakeTensorMode():
            img, pre = torch.empty((4, 3, 224, 672)), torch.empty((4, 6), dtype=torch.int64)
            lens = torch.tensor([1, 6, 3, 2], dtype=torch.int32)
            sizes = torch.tensor([[224, 672]] * 4, dtype=torch.int32)
            for want in (False, True):
                for out in (torch.ops.texocr.generate_prefix(img, pre, lens, eid, 20, -1, want),
                            torch.ops.texocr.generate_prefix_from_enc(torch.empty((4, 589, 256)), pre, None, eid, 20, 997, want),
                            torch.ops.texocr.generate_prefix_ragged(img, sizes, pre, lens, eid, 20, -1, want)):
                    toks, n, logp, plogp = out
                    assert toks.shape == (4, 20) and toks.dtype == torch.int64
                    assert n.shape == (1,) and n.dtype == torch.int64 and n.device.type == "cpu"
                    assert logp.shape == (4 if want else 0, 20) and logp.dtype == torch.float32
                    assert plogp.shape == (4 if want else 0, 6) and plogp.dtype == torch.float32
        # real calls: refused before the engine is touched (the stub has no handle)
        with pytest.raises(ValueError, match="CUDA/HIP tensor"):
            ops.generate_prefix(torch.zeros(1, 3, 16, 16), torch.zeros((1, 2), dtype=torch.int64), None, eid, 4, -1, False)
        with pytest.raises(ValueError, match=r"\(B, C, Hc, Wc\)"):
            ops.generate_prefix_ragged(torch.zeros(3, 16, 16), torch.tensor([[16, 16]], dtype=torch.int32), torch.zeros((1, 2), dtype=torch.int64),
                                       None, eid, 4, -1, False)
    finally:
        ops.unregister_engine(eid)


def test_facade_refusals_need_no_engine():
    from texocr_amd.model import OCRModel
    stub = types.SimpleNamespace()
    pre = torch.zeros((1, 2), dtype=torch.int64)
    img = torch.zeros(1, 3, 16, 16)
    stub._generate_prefix = types.MethodType(OCRModel._generate_prefix, stub)
    with pytest.raises(ValueError, match="prefix= is not available with beam search"):
        OCRModel.generate(stub, img, 4, prefix=pre, beam=2)
    with pytest.raises(ValueError, match="prefix= is not available with return_logits"):
        OCRModel.generate(stub, img, 4, prefix=pre, return_logits=True)
    with pytest.raises(ValueError, match="prefix_len needs prefix"):
        OCRModel.generate(stub, img, 4, prefix_len=[1])
    with pytest.raises(ValueError, match="prefix_len needs prefix"):
        OCRModel.generate_ragged(stub, [img[0]], 4, prefix_len=[1])
    with pytest.raises(ValueError, match=r"prefix must be an int64 tensor of shape \(B, P\)"):
        OCRModel.generate(stub, img, 4, prefix=torch.zeros((2, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="prefix must be an int64"):
        OCRModel.generate(stub, img, 4, prefix=pre.float())
