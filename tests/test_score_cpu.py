"""No-GPU checks of teacher-forced scoring: the CPU oracle reproduces the fixtures captured from the reference
(tests/capture_score_golden.py -> tests/golden/score_*), which pins the test-side reference of tests/test_gpu_score.py as
test_oracle_golden.py pins it for the other paths; the two new C entry points validate their arguments before any HIP call; the
arithmetic of the Score tuple on hand-made tensors."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from oracle import cpu_ref
from texocr_amd import synth
from texocr_amd.config import Dims

CASES = ["score_tiny", "score_cfg1", "score_ragged"]


def oracle_logits(meta, g):
    d = Dims(**meta["dims"])
    sd = cpu_ref.to_torch_sd(synth.synth_state_dict(d, meta["weight_seed"]))
    img = torch.from_numpy(synth.synth_images(*meta["image_shape"], seed=meta["image_seed"]))
    trg = torch.from_numpy(g["trg"].astype(np.int64))
    mask = torch.from_numpy(g["mask"]).bool()
    out = cpu_ref.decoder_net(sd, trg[:, :-1], cpu_ref.encode(sd, img), mask=mask[:, :-1])
    return trg, mask, out


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_the_reference_scores(name):
    meta, g = load_golden(name)
    trg, mask, out = oracle_logits(meta, g)
    assert trg.shape[1] == meta["L"] and out.shape[:2] == g["logp"].shape
    valid = (mask[:, :-1] & mask[:, 1:]).numpy()
    assert valid.all() != meta["padded"]
    lsm = torch.log_softmax(out, -1)
    logp = lsm.gather(-1, trg[:, 1:, None])[..., 0].numpy()
    top1 = out.argmax(-1)
    top1_logp = lsm.gather(-1, top1[..., None])[..., 0].numpy()
    assert float(np.abs(logp - g["logp"])[valid].max()) < 1e-5
    assert float(np.abs(top1_logp - g["top1_logp"])[valid].max()) < 1e-5
    top2 = out.topk(2, -1).values
    assert float(np.abs((top2[..., 0] - top2[..., 1]).numpy() - g["margin"])[valid].max()) < 1e-5
    decided = valid & (g["margin"] >= 2e-5)
    assert np.array_equal(top1.numpy()[decided], g["top1"].astype(np.int64)[decided])
    if not meta["padded"]:
        # model/decoder.py:140: the reference's loss is the plain mean over every position
        loss = float(F.cross_entropy(out.transpose(1, 2), trg[:, 1:]))
        assert abs(loss - meta["loss"]) < 1e-5, (loss, meta["loss"])
        assert abs(float(-g["logp"].astype(np.float64).mean()) - meta["loss"]) < 1e-5      # the fixture agrees with itself


def test_ragged_fixture_is_ragged():
    meta, g = load_golden("score_ragged")
    d = Dims(**meta["dims"])
    lengths = g["mask"].sum(1)
    assert len(set(lengths.tolist())) == 3 and lengths.max() == meta["L"]
    assert np.array_equal(g["mask"] != 0, g["trg"] != d.pad)                             # make_trg_mask


def test_score_entry_points_refuse_null_and_bad_length_without_gpu():
    from texocr_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.txo_decode_score(None, None, 4, None, None, None, None) == _lib.TXO_E_INVALID
    assert lib.txo_score(None, None, 1, 3, 16, 16, None, None, 4, None, None, None, None) == _lib.TXO_E_INVALID
    # a non-null handle is not dereferenced before the token pointer is checked
    fake = C.c_void_p(8)
    assert lib.txo_decode_score(fake, None, 4, None, None, None, None) == _lib.TXO_E_INVALID
    assert lib.txo_score(fake, None, 1, 3, 16, 16, None, None, 4, None, None, None, None) == _lib.TXO_E_INVALID
    with pytest.raises(ValueError):
        _lib.check(lib.txo_decode_score(None, None, 1, None, None, None, None))


def test_score_summary_arithmetic():
    from texocr_amd.model import Score, score_summary
    pad = 9
    trg = torch.tensor([[7, 1, 2, 3], [7, 4, pad, pad]])
    mask = trg != pad
    logp = torch.tensor([[-0.5, -1.0, -2.0], [-0.25, -100.0, float("nan")]])           # values outside `valid` must not matter
    top1 = torch.tensor([[1, 5, 3], [4, pad, pad]])
    top1_logp = torch.tensor([[-0.5, -0.1, -2.0], [-0.25, -0.1, -0.1]])
    s = score_summary(logp, top1, top1_logp, trg, mask)
    assert isinstance(s, Score) and s._fields == ("logp", "top1", "top1_logp", "valid", "nll", "loss", "token_acc")
    assert s.valid.tolist() == [[True, True, True], [True, False, False]]
    assert s.nll.tolist() == [3.5, 0.25]
    assert s.loss.ndim == 0 and math.isclose(float(s.loss), 3.75 / 4, rel_tol=1e-6)
    assert s.token_acc.ndim == 0 and math.isclose(float(s.token_acc), 3 / 4, rel_tol=1e-6)
    assert s.logp is logp and s.top1 is top1 and s.top1_logp is top1_logp
    # no padding: loss is the mean of -logp, the reference's F.cross_entropy
    full = score_summary(logp[:1], top1[:1], top1_logp[:1], trg[:1], mask[:1])
    assert math.isclose(float(full.loss), 3.5 / 3, rel_tol=1e-6) and math.isclose(float(full.token_acc), 2 / 3, rel_tol=1e-6)
