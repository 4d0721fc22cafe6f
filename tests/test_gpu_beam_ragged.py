"""GPU tests of OCRModel.beam_search (txo_beam_search / txo_beam_search_ragged; csrc/step.h: beam_select_kernel<true>, beam_finish_kernel):
beam search over a fixed batch or a list of pictures of different sizes, every beam with its score, its length and the log-probability of
each of its tokens.

References and bounds (none comes from the code under test):
- generate(beam=k, return_beams=True) of the same engine: tokens and scores bit for bit (the search is the same loop);
- the float of every position: summed left to right in float32 it IS the score, bit for bit; against float64 (beam_ref.prefix_logp64 on the
  beam's own prefix) within FP32_LOGP = 2e-4 in fp32 (tests/test_gpu_score.py) and 2 x BF16_BOUND["logits"] in bf16; against model.score()
  within the same bounds;
- a ragged row against the solo call of the same engine: bit for bit in fp32;
- bf16: every step of the ragged call replayed in float64 per picture (beam_ref.replay_pairs, the eps rule of tests/test_gpu_beam.py).

Shapes: T = the w128 case on TINY_SIZES (2 to 65 keys, one picture twice); P = Dims(canvas=224) on P_SIZES (197 keys: more than one fp32
pass of the cross attention, beside 2-key pictures); vocabularies 1000 / 1100 are the two paths of beam_select_kernel."""
import ctypes as C
import dataclasses
import json
import math
import os

import numpy as np
import pytest
import torch

import beam_ref as br
import ref64
from gpu_harness import BF16_BOUND, SHAPE_CASES, build, first_eos, knobs, rgb_images
from test_gpu_logp import FP32_LOGP, TINY_SIZES
from texocr_amd import _lib, ops, synth
from texocr_amd._lib import Q_LAST_LATENT, Q_LAST_RAGGED, Q_LAST_ROW_RANGES
from texocr_amd.config import Dims

pytestmark = pytest.mark.gpu

T = SHAPE_CASES["w128"][0]
P_SIZES = [(224, 224), (16, 16), (64, 96), (16, 16), (224, 32)]           # 197, 2, 25, 2, 29 keys
N_T, N_P = 24, 20                                                          # positions decoded
SEED_T, SEED_P = 3, 0                                                      # weight seeds (EOS below belongs to them)


def _dims(shape):
    return T if shape == "T" else Dims(canvas=224, vocab=int(shape[1:]))


def _case(shape, max_batch, dtype="fp32", **kw):
    """(dims, weights, model, pictures, positions) of shape 'T' / 'P1000' / 'P1100'"""
    d = _dims(shape)
    sizes, seed, n = (TINY_SIZES, SEED_T, N_T) if shape == "T" else (P_SIZES, SEED_P, N_P)
    d, sd, m = build(d, seed=seed, dtype=dtype, max_batch=max_batch, **kw)
    images = [torch.from_numpy(synth.synth_images(1, 3, h, w, seed=200 + i))[0].cuda() for i, (h, w) in enumerate(sizes)]
    if shape == "T":
        images[5] = images[1].clone()
    else:
        images[3] = images[3] * 0.5                                        # (the two 2-key pictures differ)
    return d, sd, m, images, n


# eos per (shape, k): a frequent token of the eos-free best beams, as tests/test_gpu_beam.py chooses it -- the most frequent one under which
# the pictures finish (every beam holds eos) at different positions and at least one does not finish inside n.  Found once with
# generate(beam=k) on each picture alone on the MI355X (2026-10-19; it was the most frequent token every time) and fixed here.
EOS = {("T", 1): 183, ("T", 3): 183, ("T", 5): 183, ("T", 8): 183, ("P1000", 1): 125, ("P1000", 3): 690, ("P1000", 8): 523,
       ("P1100", 1): 504, ("P1100", 3): 690, ("P1100", 8): 523}


def _eos_case(m, images, shape, k, n):
    """sets EOS[shape, k] on the model and asserts the condition on the INPUTS the tests rely on, with generate(beam=k) on each picture alone
    (the search as it was before beam_search existed): the pictures' last positions differ, one finishes early, one not inside n"""
    eos = m.eos_token = EOS[shape, k]
    solo = [m.generate(im[None], n, beam=k, return_beams=True)[0] for im in images]
    steps = [int(t.shape[2]) for t in solo]
    unfinished = [not bool((t == eos).any(2).all()) for t in solo]
    print(f"eos {eos}: steps per picture {steps}, unfinished {unfinished}")
    assert len(set(steps)) >= 2 and min(steps) < n and any(unfinished), (eos, steps, unfinished)
    return eos


def _host_lengths(tokens, eos):
    tokens = tokens.cpu().numpy()
    n = tokens.shape[-1]
    f = np.array(first_eos(tokens.reshape(-1, n), -1 if eos is None else eos)).reshape(tokens.shape[:-1])
    return np.where(f < 0, n, f + 1).astype(np.int32)


def _equal(a, b, cols=None):
    """two Beams bit for bit (over the first `cols` columns)"""
    ok = torch.equal(a.tokens[..., :cols], b.tokens[..., :cols]) and torch.equal(a.scores, b.scores) and torch.equal(a.lengths, b.lengths)
    if a.logp is not None and b.logp is not None:
        ok = ok and torch.equal(a.logp[..., :cols], b.logp[..., :cols])
    return ok


# ---- 1. the same search as generate(beam=k) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("vocab", [1000, 1100], ids=["rows_in_registers", "general_path"])
def test_same_search_as_generate_beam(vocab, k):
    d, sd, m = build(Dims(canvas=224, vocab=vocab), seed=0, max_batch=3 * 8)
    img = torch.from_numpy(synth.synth_images(3, 3, 64, 96, seed=41)).cuda()
    m.eos_token = None
    greedy = m.generate(img, N_P)
    for eos in (None, int(greedy[0, 5])):
        m.eos_token = eos
        toks, scores = m.generate(img, N_P, beam=k, return_beams=True)
        for want_logp in (False, True):
            got = m.beam_search(img, k, N_P, return_logp=want_logp)
            assert got.tokens.shape == toks.shape and got.scores.shape == (3, k) and got.lengths.dtype == torch.int32
            assert torch.equal(got.tokens, toks) and torch.equal(got.scores, scores), (eos, want_logp)
            assert (got.logp is None) == (not want_logp)
        again, s2 = m.generate(img, N_P, beam=k, return_beams=True)        # and generate(beam=) behind it is what it was
        assert torch.equal(again, toks) and torch.equal(s2, scores)
        if k == 1 and eos is None:
            assert torch.equal(got.tokens[:, 0], greedy)


# ---- 2. log-probabilities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("vocab", [200, 1100], ids=["rows_in_registers", "general_path"])
def test_logp_sums_to_the_score_and_matches_float64(vocab, dtype):
    d = dataclasses.replace(T, vocab=vocab, bos=vocab - 2, eos=vocab - 3, pad=vocab - 1)
    k, B, n = 3, 4, 14
    d, sd, m = build(d, seed=SEED_T, dtype=dtype, max_batch=B * k)
    img = rgb_images(B, 48, 80, 900)
    s64 = ref64.sd64(sd)
    enc64 = ref64.encode(s64, img)
    bound = FP32_LOGP if dtype == "fp32" else 2 * BF16_BOUND["logits"]
    # (the most frequent token of the eos-free best beams on the MI355X, 2026-10-19, fp32 and bf16 alike; that a beam ends early is asserted below)
    for eos in (None, {200: 16, 1100: 610}[vocab]):
        m.eos_token = eos
        got = m.beam_search(img.cuda(), k, n, return_logp=True)
        toks, logp, scores, lengths = got.tokens.cpu(), got.logp.cpu(), got.scores.cpu().numpy(), got.lengths.cpu().numpy()
        steps = toks.shape[2]
        # the search added exactly these floats in this order
        acc = np.zeros((B, k), np.float32)
        for t in range(steps):
            acc = (acc + logp[:, :, t].numpy()).astype(np.float32)
        assert np.array_equal(acc.view(np.uint32), scores.view(np.uint32)), (eos, acc, scores)
        assert np.array_equal(lengths, _host_lengths(toks, eos))
        behind = torch.arange(steps)[None, None, :] >= torch.from_numpy(lengths.astype(np.int64))[..., None]
        assert bool((logp[behind] == 0.0).all()) and (eos is None or bool((toks[behind] == eos).all()))
        if eos is not None:
            assert bool(behind.any()), "no beam finished early: nothing behind a length was checked"
        # float64 at the beam's own prefix, every position of every beam
        e64 = 0.0
        for t in range(steps):
            lp64 = br.prefix_logp64(s64, enc64, d.bos, toks[:, :, :t])                     # (B, k, V)
            want = np.take_along_axis(lp64, toks[:, :, t].numpy()[..., None], 2)[..., 0]
            live = ~behind[:, :, t].numpy()
            e64 = max(e64, float(np.abs(logp[:, :, t].numpy().astype(np.float64) - want)[live].max()) if live.any() else 0.0)
        # the engine's second pass: score() on [bos] + the beams
        rows = toks.reshape(B * k, steps).cuda()
        trg = torch.cat([torch.full((B * k, 1), d.bos, dtype=torch.int64, device="cuda"), rows], 1)
        s = m.score(img.cuda().repeat_interleave(k, 0), trg, mask=torch.ones_like(trg, dtype=torch.bool))
        live = ~behind.reshape(B * k, steps)
        esc = float((s.logp.cpu() - logp.reshape(B * k, steps))[live].abs().max())
        print(f"beam logp V={vocab} {dtype} eos={eos}: {steps} steps, max |d| vs float64 {e64:.3e}, vs score() {esc:.3e} (bound {bound:.1e})")
        assert e64 <= bound and esc <= bound, (e64, esc)


# ---- 3. a ragged row equals the solo call --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("shape", ["T", "P1000", "P1100"])
def test_ragged_row_equals_the_solo_call(shape, k):
    d, sd, m, images, n = _case(shape, max_batch=len(TINY_SIZES if shape == "T" else P_SIZES) * k)
    for eos in (None, "frequent"):
        eos = _eos_case(m, images, shape, k, n) if eos else None
        m.eos_token = eos
        rag = m.beam_search(images, k, n, return_logp=True)
        assert m._engine.query(Q_LAST_RAGGED) == 1 and m._engine.query(Q_LAST_LATENT) == 0
        assert rag.tokens.shape[:2] == (len(images), k) and rag.logp.shape == rag.tokens.shape
        assert np.array_equal(rag.lengths.cpu().numpy(), _host_lengths(rag.tokens, eos))
        for b, im in enumerate(images):
            solo = m.beam_search(im[None], k, n, return_logp=True)
            ns = solo.tokens.shape[2]
            assert ns <= rag.tokens.shape[2]
            assert torch.equal(rag.tokens[b, :, :ns], solo.tokens[0]), (b, eos)
            assert torch.equal(rag.scores[b], solo.scores[0]) and torch.equal(rag.lengths[b], solo.lengths[0]), (b, eos)
            assert torch.equal(rag.logp[b, :, :ns], solo.logp[0]), (b, eos, float((rag.logp[b, :, :ns] - solo.logp[0]).abs().max()))
            if ns < rag.tokens.shape[2]:
                assert bool((rag.tokens[b, :, ns:] == eos).all()) and bool((rag.logp[b, :, ns:] == 0.0).all()), b
        dup = (5, 1) if shape == "T" else None
        if dup:
            assert all(torch.equal(x[dup[0]], x[dup[1]]) for x in (rag.tokens, rag.scores, rag.lengths, rag.logp))


# ---- 4. equal sizes ------------------------------------------------------------------------------------------------------------------
def test_ragged_call_on_equal_sizes_equals_the_fixed_shape_call():
    d, sd, m = build(T, seed=SEED_T, max_batch=4 * 3)
    img = rgb_images(4, 48, 80, 900).cuda()
    for eos in (None, int(m.beam_search(img, 3, N_T).tokens[0, 0, 4])):
        m.eos_token = eos
        fixed = m.beam_search(img, 3, N_T, return_logp=True)
        assert m._engine.query(Q_LAST_RAGGED) == 0
        rag = m.beam_search(list(img), 3, N_T, return_logp=True)
        assert m._engine.query(Q_LAST_RAGGED) == 1
        assert rag.tokens.shape == fixed.tokens.shape and _equal(rag, fixed), eos


# ---- 5. two row ranges ---------------------------------------------------------------------------------------------------------------
def test_two_row_ranges_equal_one():
    """P on TXO_LANES=2: 5 pictures split 3 + 2, the second range's key counts (2, 29) differ from the first's (197, 2, 25), so key
    counts taken from the wrong offset of the per-image table show"""
    d, sd, m, images, n = _case("P1000", max_batch=5 * 3)
    for eos in (None, "frequent"):
        eos = _eos_case(m, images, "P1000", 3, n) if eos else None
        m.eos_token = eos
        with knobs(TXO_LANES=1):
            one = m.beam_search(images, 3, n, return_logp=True)
            assert m._engine.query(Q_LAST_ROW_RANGES) == 1
        with knobs(TXO_LANES=2):
            two = m.beam_search(images, 3, n, return_logp=True)
            assert m._engine.query(Q_LAST_ROW_RANGES) == 2
        assert two.tokens.shape == one.tokens.shape and _equal(one, two), eos


# ---- 6. nothing outside the corner is read -------------------------------------------------------------------------------------------
def _fill_outside(box, sizes, value):
    out = torch.full_like(box, value)
    for b, (h, w) in enumerate(sizes.tolist()):
        out[b, :, :h, :w] = box[b, :, :h, :w]
    return out


def test_nothing_outside_the_corner_is_read():
    d, sd, m, images, n = _case("T", max_batch=len(TINY_SIZES) * 3)
    m.eos_token = None
    eng = m._engine
    box, sizes = ops.pack_ragged(images)

    def run(container):
        return [x.clone() for x in torch.ops.texocr.beam_search_ragged(container, sizes, eng.id, 3, n, -1, True, 0.0)[:4]]

    base = run(box)
    assert bool(torch.isfinite(base[1]).all()) and bool(torch.isfinite(base[3]).all())
    for value in (0.0, 1e30, float("nan")):
        for a, b, name in zip(base, run(_fill_outside(box, sizes, value)), ("tokens", "scores", "lengths", "logp")):
            assert torch.equal(a, b), f"{name} changed with {value} outside the corners"
    bad = box.clone()
    bad[2, 0, 3, 5] = float("nan")                            # inside picture 2 (16x16)
    others = [r for r in range(len(images) * 3) if r // 3 != 2]
    for a, b, name in zip(base, run(bad), ("tokens", "scores", "lengths", "logp")):
        assert torch.equal(a[others], b[others]), f"{name} of another picture changed with a NaN inside picture 2"


# ---- 7. bf16: every step of the ragged call pinned to float64 ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["T", "P1000"])
def test_bf16_ragged_steps_replayed_in_float64(shape):
    d, sd, m, images, n = _case(shape, max_batch=len(TINY_SIZES if shape == "T" else P_SIZES) * 3, dtype="bf16")
    k, pairs = 3, (0, 1, 2, 15, 16, 17)
    m.eos_token = None
    s64 = ref64.sd64(sd)
    states = {}
    for length in sorted({p + dl for p in pairs for dl in (0, 1) if p + dl > 0}):
        r = m.beam_search(images, k, length)
        assert m._engine.query(Q_LAST_RAGGED) == 1 and r.tokens.shape == (len(images), k, length)
        states[length] = (r.tokens.cpu().numpy(), r.scores.cpu().numpy())
    eps = lambda a, b: 2 * BF16_BOUND["logits"]                # tests/test_gpu_beam.py: the bf16 eps rule
    worst = 0.0
    for b, im in enumerate(images):                            # every picture against the float64 run of that picture alone
        enc64 = ref64.encode(s64, im[None].cpu(), grid_w=d.grid)
        own = {length: (t[b:b + 1], s[b:b + 1]) for length, (t, s) in states.items()}
        rep = br.replay_pairs(s64, enc64, d.bos, None, own, pairs, eps)
        assert rep.steps == len(pairs)
        worst = max(worst, rep.inc_err)
    # ragged against solo bits: measured, printed and asserted.  Measured on MI355X, 2026-10-19: 0 of 7 (T) and 0 of 5 (P1000) pictures
    # differ at 18 positions, so equality is asserted; the float64 replay above stands on its own.
    diff = 0
    last = max(states)
    for b, im in enumerate(images):
        solo = m.beam_search(im[None], k, last)
        diff += int(not (np.array_equal(solo.tokens[0].cpu().numpy(), states[last][0][b]) and
                         np.array_equal(solo.scores[0].cpu().numpy(), states[last][1][b])))
    print(f"bf16 ragged beam search {shape}: max |score increment - float64 log-prob| {worst:.3e} (eps {eps(0, 0):.3e}); pictures whose "
          f"ragged row differs from the solo call's bits at {last} positions: {diff} of {len(images)}")
    assert diff == 0


# ---- 8. length_alpha -----------------------------------------------------------------------------------------------------------------
def _check_alpha(m, images, k, n, base, alpha):
    """the order under length_alpha against the host's; returns how many pictures change their order"""
    got = m.beam_search(images, k, n, return_logp=True, length_alpha=alpha)
    sc, ln = base.scores.cpu().numpy(), base.lengths.cpu().numpy()
    key = sc.astype(np.float64) / ln.astype(np.float32).astype(np.float64) ** alpha
    moved = 0
    for b in range(len(images)):
        kb = key[b]
        for i in range(k):
            for j in range(i + 1, k):
                assert abs(kb[i] - kb[j]) > 1e-6 * max(abs(kb[i]), abs(kb[j])), ("a near-tie in the inputs: pick other seeds", b, i, j, kb)
        order = np.argsort(-kb, kind="stable")
        moved += int(not np.array_equal(order, np.arange(k)))
        idx = torch.from_numpy(order).cuda()
        assert torch.equal(got.tokens[b], base.tokens[b][idx]), (b, order)
        assert torch.equal(got.scores[b], base.scores[b][idx]) and torch.equal(got.lengths[b], base.lengths[b][idx])
        assert torch.equal(got.logp[b], base.logp[b][idx])
    print(f"length_alpha {alpha}: {moved} of {len(images)} pictures change their order")
    return moved


def test_length_alpha_reorders_and_nothing_else():
    """alpha in {0.6, 1.0}: the beams of alpha = 0 in the host's stable order of score / length ** alpha, scores, lengths and logp moving
    with them.  A condition on the inputs: over the two alphas at least one picture changes its order (else nothing was ranked)."""
    d, sd, m, images, n = _case("T", max_batch=len(TINY_SIZES) * 5)
    k = 5
    _eos_case(m, images, "T", k, n)
    base = m.beam_search(images, k, n, return_logp=True)
    moved = [_check_alpha(m, images, k, n, base, alpha) for alpha in (0.6, 1.0)]
    assert sum(moved) >= 1, "no picture's order changed under either alpha: the ranking was not exercised"


# ---- 9. hybrid, opt-in ---------------------------------------------------------------------------------------------------------------
def test_hybrid_front_end_needs_the_switch_and_then_equals_solo():
    import test_gpu_hybrid_ragged as hr
    images = hr.cuda([hr._image(0, 32, 256), hr._image(1, 16, 16)])
    off = hr.model("fp32", max_batch=4, on=False)
    with pytest.raises(ValueError, match="hybrid front end"):
        off.beam_search(images, 2, 8)
    m = hr.model("fp32", max_batch=4)
    rag = m.beam_search(images, 2, 8, return_logp=True)
    for b, im in enumerate(images):
        solo = m.beam_search(im[None], 2, 8, return_logp=True)
        assert all(torch.equal(x[b], y[0]) for x, y in zip(rag, solo)), b


# ---- 10. refusals and state ----------------------------------------------------------------------------------------------------------
def _abi(eng, img, beams, max_len, alpha=0.0, sizes=None, null_out=False, null_tokens=False):
    """the C ABI's return code and message; outputs sized for a valid call"""
    eng._ensure()
    B, Cc, H, W = img.shape
    rows = max(1, B * max(1, min(beams, 8)))
    toks = torch.zeros((rows, max(max_len, 1)), dtype=torch.int64, device="cuda")
    out = _lib.TxoBeamOut(None if null_tokens else toks.data_ptr(), None, None, None, alpha)
    n = C.c_int32(0)
    po = None if null_out else C.byref(out)
    with torch.cuda.device(eng.device):
        if sizes is None:
            rc = eng.lib.txo_beam_search(eng.handle, img.data_ptr(), B, Cc, H, W, beams, max_len, -1, po, C.byref(n), None)
        else:
            s = torch.tensor(sizes, dtype=torch.int32)
            rc = eng.lib.txo_beam_search_ragged(eng.handle, img.data_ptr(), B, Cc, H, W, ops._i32p(s), beams, max_len, -1, po, C.byref(n), None)
    torch.cuda.synchronize()
    return rc, eng.lib.txo_last_error().decode()


def test_refusals_through_the_c_abi_and_the_facade():
    d, sd, m = build(T, seed=SEED_T, max_batch=6)
    eng = m._engine
    img = rgb_images(2, 32, 48, 5).cuda()
    same = [(32, 48), (32, 48)]
    cases = [(dict(beams=0, max_len=8), "beams must be in"), (dict(beams=9, max_len=8), "beams must be in"),
             (dict(beams=4, max_len=8), "images * beams"), (dict(beams=2, max_len=0), "max_len"),
             (dict(beams=2, max_len=d.max_len + 1), "max_len"), (dict(beams=2, max_len=8, null_out=True), "null out"),
             (dict(beams=2, max_len=8, null_tokens=True), "null out"), (dict(beams=2, max_len=8, alpha=-0.5), "length_alpha"),
             (dict(beams=2, max_len=8, alpha=float("nan")), "length_alpha"), (dict(beams=2, max_len=8, alpha=float("inf")), "length_alpha")]
    for kw, word in cases:
        for sizes in (None, same):
            rc, msg = _abi(eng, img, sizes=sizes, **kw)
            assert rc == _lib.TXO_E_INVALID and word in msg, (kw, sizes, rc, msg)
    rc, msg = _abi(eng, img, 2, 8, sizes=[(32, 48), (24, 48)])             # a ragged refusal: a side that is no multiple of 16
    assert rc == _lib.TXO_E_INVALID and "multiples of 16" in msg
    for kw in (dict(beams=0), dict(beams=9), dict(beams=4), dict(max_len=0), dict(max_len=d.max_len + 1), dict(length_alpha=-1.0),
               dict(length_alpha=float("nan")), dict(length_alpha=float("inf")), dict(beams=2.0)):
        args = dict(beams=2, max_len=8)
        args.update(kw)
        la = args.pop("length_alpha", 0.0)
        for src in (img, list(img)):
            with pytest.raises(ValueError, match="beam search"):
                m.beam_search(src, args["beams"], args["max_len"], length_alpha=la)
    with pytest.raises(ValueError, match="return_logp is not available with beam search"):
        m.generate(img, 8, beam=2, return_logp=True)                       # generate(beam=) keeps its refusal
    assert _abi(eng, img, 2, 8)[0] == 0 and _abi(eng, img, 2, 8, sizes=same)[0] == 0      # and the valid calls pass


def test_a_positional_table_beyond_1024_is_refused():
    d = dataclasses.replace(T, max_len=1025)
    _, _, m = build(d, seed=SEED_T, max_batch=2)
    img = rgb_images(1, 32, 48, 5).cuda()
    for sizes in (None, [(32, 48)]):
        rc, msg = _abi(m._engine, img, 2, 8, sizes=sizes)
        assert rc == _lib.TXO_E_INVALID and "1024" in msg, (rc, msg)
    with pytest.raises(ValueError, match="1024"):
        m.beam_search(img, 2, 8)


def test_latent_form_refuses_the_ragged_call_only():
    d, sd, m = build(SHAPE_CASES["w64_h4"][0], seed=1, max_batch=4, latent=1)
    img = rgb_images(2, 32, 48, 5).cuda()
    m.eos_token = None
    fixed = m.beam_search(img, 2, 8)
    assert m._engine.query(Q_LAST_LATENT) == 1 and torch.equal(fixed.tokens, m.generate(img, 8, beam=2, return_beams=True)[0])
    with pytest.raises(ValueError, match="TXO_LATENT=1"):
        m.beam_search(list(img), 2, 8)


def test_state_behind_a_ragged_beam_search():
    d, sd, m, images, n = _case("T", max_batch=len(TINY_SIZES) * 2)
    m.eos_token = None
    eng = m._engine
    x = rgb_images(3, 32, 48, 10).cuda()
    before = (m.generate(x, 8), m.generate(x, 8, beam=2, return_beams=True), m.generate_ragged(images, 8))
    m.beam_search(images, 2, n, return_logp=True)
    with pytest.raises(RuntimeError, match="needs a session"):             # no ragged session is open behind it, and the binding knows
        eng.decode_step(0, torch.full((7,), d.bos, dtype=torch.int64, device="cuda"))
    nxt = torch.empty((7,), dtype=torch.int64, device="cuda")
    with torch.cuda.device(eng.device):
        assert eng.lib.txo_decode_step(eng.handle, None, 0, None, nxt.data_ptr(), None) == _lib.TXO_E_STATE
    m.beam_search(images, 2, n)
    after = (m.generate(x, 8), m.generate(x, 8, beam=2, return_beams=True), m.generate_ragged(images, 8))
    assert torch.equal(before[0], after[0]) and torch.equal(before[2], after[2])
    assert torch.equal(before[1][0], after[1][0]) and torch.equal(before[1][1], after[1][1])
    # the fixed-shape call leaves one row per image, as generate(beam=) does (tests/test_gpu_session.py)
    eng.decode_begin(m.encoder(x[:2]))
    m.beam_search(x, 2, 8)
    logits, tok = eng.decode_step(0, torch.full((3,), d.bos, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    assert logits.shape == (3, d.vocab) and tok.shape == (3,) and int(tok.min()) >= 0 and int(tok.max()) < d.vocab


# ---- 11. wrapper ---------------------------------------------------------------------------------------------------------------------
def test_wrapper_decodes_with_beams(tmp_path):
    from PIL import Image
    from texocr_amd.config import default_config
    from texocr_amd.tokenizer import RegExTokenizer
    from texocr_amd.wrapper import TeXOCRWrapper
    v = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tokenizer_vocab_1k.json")))
    RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"]).save(str(tmp_path / "vocab.txt"))
    cfg = default_config(img_size=[64, 256], max_length=32, in_channels=1,
                         encoder={"embed_dim": 64, "heads": 2, "num_layers": 1}, decoder={"embed_dim": 64, "heads": 2, "num_layers": 2})
    cfg["tokenizer_path"] = str(tmp_path / "vocab.txt")
    rng = np.random.RandomState(0)
    pil = []
    for wd, ht in [(200, 40), (30, 30), (250, 64), (30, 30)]:
        a = np.full((ht, wd, 3), 255, dtype=np.uint8)
        a[rng.randint(0, ht, 40), rng.randint(0, wd, 40)] = rng.randint(0, 120, (40, 1))
        pil.append(Image.fromarray(a))
    results = []
    for max_batch in (7, 9):                                               # chunks of 2 and of 3 pictures
        w = TeXOCRWrapper(cfg, max_batch=max_batch)
        w.model.load_state_dict(synth.synth_state_dict(w.dims, 5))
        got = w.batch(pil, max_len=20, decode="beam", beams=3, return_logp=True)
        results.append(got)
        assert len(got) == 4 > max_batch // 3
        for im, g in zip(pil, got):
            one = w(im, max_len=20, decode="beam", beams=3, return_logp=True)
            assert len(one) == 3 and one[0] == g[0] and one[1] == g[1] and one[2] == g[2], (one, g)
            assert len(g[2]) == len(g[0]) and all(isinstance(x, float) and x <= 0.0 for x in g[2])
        assert w.batch(pil, max_len=20, decode="beam", beams=3) == [g[:2] for g in got]
    assert results[0] == results[1]
    aligned = w.batch(pil, max_len=20, decode="beam", beams=3, return_align=True)
    for im, g, a in zip(pil, results[1], aligned):
        gh, gw = math.ceil(im.size[1] / 16), math.ceil(im.size[0] / 16)
        assert a[:2] == g[:2] and tuple(a[2].shape) == (len(g[0]), gh, gw)
    one = w(pil[0], max_len=20, decode="beam", beams=3, return_align=True)
    assert one[:2] == results[1][0][:2] and tuple(one[2].shape) == tuple(aligned[0][2].shape)
    with pytest.raises(ValueError, match="max_batch"):
        TeXOCRWrapper(cfg, max_batch=2).batch(pil, decode="beam", beams=3)
    with pytest.raises(ValueError, match="max_batch"):
        TeXOCRWrapper(cfg, max_batch=2)(pil[0], decode="beam", beams=3)
