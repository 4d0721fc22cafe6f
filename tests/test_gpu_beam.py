"""GPU tests of beam search (BASELINE config 5 asks for it; the reference has none, SURVEY D3: a build extension).

Convention: parity is anchored at beams=1 == greedy and at the oracle's independent CPU restatement of the same definition (tokens
exact, scores within 2e-3 in fp32); one row range against two bit for bit."""
import numpy as np
import pytest
import torch

from gpu_harness import build, knobs, oracle
from texocr_amd import synth
from texocr_amd._lib import Q_LAST_LATENT, Q_LAST_ROW_RANGES
from texocr_amd.config import Dims

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("latent", [None, 1], ids=["kv_form", "latent_form"])
@pytest.mark.parametrize("vocab", [1000, 1100], ids=["rows_in_registers", "general_path"])
def test_beam_search_extension(vocab, latent):
    """BASELINE config 5 asks for beam search; the reference has none, so parity is anchored at
    beams=1 == greedy, plus agreement with the oracle's independent CPU restatement of the same definition.
    Both forms of beam_select_kernel (csrc/step.h): an image's k rows in registers up to 1024 entries, the general path beyond."""
    cpu_ref = oracle()
    d = Dims(canvas=224, vocab=vocab)
    # latent_form: the cross attention against the raw encoder rows, an image's k beams as ONE row of k * heads heads (16 per tile)
    d, sd, m = build(d, seed=0, max_batch=12, latent=latent)
    img = torch.from_numpy(synth.synth_images(3, 3, 64, 96, seed=41))
    m.eos_token = None
    greedy = m.generate(img.cuda(), 24)
    assert torch.equal(m.generate(img.cuda(), 24, beam=1), greedy)
    assert m._engine.query(Q_LAST_LATENT) == (1 if latent else 0)
    sdt = cpu_ref.to_torch_sd(sd)
    enc = cpu_ref.encode(sdt, img)
    for k, eos in ((4, None), (3, int(greedy[0, 5]))):
        m.eos_token = eos
        toks, scores = m.generate(img.cuda(), 24, beam=k, return_beams=True)
        ref_t, ref_s = cpu_ref.beam_search_cached(sdt, enc, d.bos, eos, 24, k)
        assert toks.shape[:2] == (3, k) and toks.shape[2] == ref_t.shape[2]
        np.testing.assert_allclose(scores.cpu().numpy(), ref_s.numpy(), atol=2e-3)
        assert bool((scores[:, :-1] >= scores[:, 1:]).all())                  # best first
        assert torch.equal(toks.cpu(), ref_t), (k, eos)
        best = m.generate(img.cuda(), 24, beam=k)
        assert torch.equal(best, toks[:, 0])
        assert torch.equal(m.generate(img.cuda(), 24, beam=k), best)          # deterministic
        # two row ranges on two streams (the default from 256 beam rows on): ranges are whole images, slots range-local -> the same bits
        with knobs(TXO_LANES=2):
            toks2, scores2 = m.generate(img.cuda(), 24, beam=k, return_beams=True)
            assert m._engine.query(Q_LAST_ROW_RANGES) == 2
        assert torch.equal(toks2, toks) and torch.equal(scores2, scores)
    with pytest.raises(ValueError):
        m.generate(img.cuda(), 24, beam=9)
    with pytest.raises(ValueError):
        m.generate(torch.rand(5, 3, 64, 96, device="cuda"), 24, beam=3)       # 15 rows > max_batch 12


def test_beam_search_two_row_ranges_at_300_rows_bit_identical_to_one():
    """From 256 beam rows on, beam search decodes two row ranges (whole images each) on two streams, in bf16 with the latent cross
    attention whose tiles take up to 16 heads = two beams of an image: same tokens and scores as ONE range."""
    d = Dims(canvas=224, max_len=16)
    _, _, m = build(d, seed=9, dtype="bf16", max_batch=300)
    img = torch.from_numpy(synth.synth_images(60, 3, 32, 64, seed=17)).cuda()
    m.eos_token = None
    t2, s2 = m.generate(img, 12, beam=5, return_beams=True)
    assert m._engine.query(Q_LAST_ROW_RANGES) == 2 and m._engine.query(Q_LAST_LATENT) == 1
    with knobs(TXO_LANES=1):
        t1, s1 = m.generate(img, 12, beam=5, return_beams=True)
        assert m._engine.query(Q_LAST_ROW_RANGES) == 1
    assert torch.equal(t1, t2) and torch.equal(s1, s2)
    # with an eos (the most frequent token of the best beams): finished beams repeat eos at no cost, the loop stops only when EVERY
    # range's beams are finished -- same length, same beams, same scores on one range and on two
    vals, counts = np.unique(t2[:, 0].cpu().numpy(), return_counts=True)
    m.eos_token = int(vals[counts.argmax()])
    e2 = m.generate(img, 12, beam=5, return_beams=True)
    with knobs(TXO_LANES=1):
        e1 = m.generate(img, 12, beam=5, return_beams=True)
    assert e1[0].shape == e2[0].shape and torch.equal(e1[0], e2[0]) and torch.equal(e1[1], e2[1])
    assert not torch.equal(e2[0], t2[:, :, :e2[0].shape[2]]) or e2[0].shape[2] < 12      # the eos changed something
