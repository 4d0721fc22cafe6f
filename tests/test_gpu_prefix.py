"""GPU tests of the prompted decode (include/texocr.h: txo_generate_prefix / _from_enc / _ragged; csrc/step_prefix.h): generate()'s loop
continued behind a caller's token prefix, with a length per row.

What is pinned: (1) the reference -- with equal lengths the result is decoder.generate(start_tokens)'s, the `ragged_prefix` fixture's
tokens_unmasked, through C ABI, operator and module, and equal bit for bit to the stepwise loop (same multi-position pass, same step
launches); (2) forcing what the model would pick changes nothing -- tokens and log-probabilities bit for bit those of generate() from
BOS; (3) per-row lengths against float64 (tests/prefix_ref.py), with the margin asserted at every free position; (4) eos: prefixes that
hold it, the break position, stop='row' with forced compactions; (5) both cross-attention forms, ragged batches, the decode path;
(6) the facades and every refusal before the engine's session changes.

Bounds: FP32_LOGP (tests/test_gpu_score.py) in fp32, 2 * BF16_BOUND["logits"] in bf16 (tests/test_gpu_logp.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_harness import BF16_BOUND, SHAPE_CASES, STOP_ENV, build, first_eos, images, knobs, stop_case
from texocr_amd import synth
from texocr_amd._lib import Q_LAST_COMPACTIONS, Q_LAST_LATENT, Q_LAST_PERSISTENT, Q_LAST_ROW_RANGES
from texocr_amd.config import Dims

import prefix_ref
import ref64
from test_gpu_logp import FP32_LOGP, TINY_SIZES

pytestmark = pytest.mark.gpu

W128 = SHAPE_CASES["w128"][0]                                       # vocab 200: the 16-byte branch of the token selection
W128_ODD = Dims(**{**W128.to_dict(), "vocab": 201, "bos": 199, "eos": 198, "pad": 200})   # vocab 201: its scalar branch


def _rgb(b, seed, h=64, w=96):
    return torch.from_numpy(synth.synth_images(b, 3, h, w, seed=seed))


def _launch(m, call):
    """call() on the launch path (TXO_PERSIST=0), asserting it"""
    with knobs(TXO_PERSIST=0):
        out = call()
    assert m._engine.query(Q_LAST_PERSISTENT) == 0
    return out


# ---- 1. the reference ------------------------------------------------------------------------------------------------------------
def _abi_from_enc(eng, enc, prefix, max_len, eos, lens=None):
    B, P = prefix.shape
    toks = torch.full((B, max_len), -7, dtype=torch.int64, device="cuda")
    logp = torch.full((B, max_len), float("nan"), device="cuda")
    plogp = torch.full((B, P), float("nan"), device="cuda")
    n = C.c_int32(0)
    lp = None if lens is None else (C.c_int32 * B)(*lens)
    rc = eng.lib.txo_generate_prefix_from_enc(eng.handle, enc.data_ptr(), B, enc.shape[1], prefix.data_ptr(), P, lp, max_len, eos, toks.data_ptr(),
                                              C.byref(n), logp.data_ptr(), plogp.data_ptr(), None)
    return rc, toks[:, :n.value], logp[:, :n.value], plogp


def test_equal_lengths_are_the_reference_through_every_layer():
    meta, g = load_golden("ragged_prefix")
    assert float(g["margin"].min()) >= 1e-4
    d, sd, m = build(meta, max_batch=3)
    eng = m._engine
    img = images(meta).cuda()
    enc = m.encoder(img)
    start = torch.from_numpy(g["start"].astype(np.int64)).cuda()
    n = meta["max_len"]
    want = torch.from_numpy(g["tokens_unmasked"].astype(np.int64))
    m.eos_token = None
    # C ABI
    rc, t, lp, plp = _abi_from_enc(eng, enc, start, n, -1)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(t.cpu(), want)
    assert bool(torch.isfinite(lp).all()) and bool((plp == 0).all())                  # m == P: no token is forced inside the loop
    # operator
    t2, n2, lp2, plp2 = torch.ops.texocr.generate_prefix_from_enc(enc, start, None, eng.id, n, -1, True)
    assert int(n2) == n and torch.equal(t2.cpu(), want) and torch.equal(lp2, lp)
    t3 = torch.ops.texocr.generate_prefix(img, start, None, eng.id, n, -1, False)[0]
    assert torch.equal(t3.cpu(), want)
    # module: model.generate(prefix=), decoder.generate(start_tokens) -- and the latter is the new route: return_logp works on it
    assert torch.equal(m.generate(img, n, prefix=start).cpu(), want)
    assert eng.query(Q_LAST_PERSISTENT) == 0
    assert torch.equal(m.decoder.generate(start, None, n, enc=enc).cpu(), want)
    t4, lp4, plp4 = m.decoder.generate(start, None, n, enc=enc, return_logp=True)
    assert torch.equal(t4.cpu(), want) and torch.equal(lp4, lp) and plp4.shape == start.shape
    # the stepwise loop on the same inputs: the same multi-position pass and the same step launches -> the same bits, greedy and sampled
    step = m.decoder._generate_stepwise(start, None, n, enc, None)
    assert torch.equal(step.cpu(), want)
    with eng.modes(sample=(0.7, 1234)) as sample:
        s_step = m.decoder._generate_stepwise(start, None, n, enc, sample)
    s_new = m.decoder.generate(start, None, n, temp=0.7, decode="sample", seed=1234, enc=enc)
    assert torch.equal(s_new, s_step)
    # bf16: equal to its own stepwise loop
    _, _, mb = build(meta, dtype="bf16", max_batch=3)
    encb = mb.encoder(img)
    assert torch.equal(mb.decoder.generate(start, None, n, enc=encb), mb.decoder._generate_stepwise(start, None, n, encb, None))
    # 1-d start_tokens squeeze like the reference's
    one = m.decoder.generate(start[0], None, 6, enc=enc[:1])
    assert one.shape == (6,) and torch.equal(one.cpu(), want[0, :6])


# ---- 2. forcing what the model would pick changes nothing -------------------------------------------------------------------------------
def _forced_identity(m, d, img, n, lens, **kn):
    B = img.shape[0]
    with knobs(**kn):
        toks, logp = _launch(m, lambda: m.generate(img, n, return_logp=True))
        P = max(lens)
        prefix = torch.cat([torch.full((B, 1), d.bos, dtype=torch.int64, device="cuda"), toks[:, :P - 1]], 1)
        t, lp, plp = _launch(m, lambda: m.generate(img, n, prefix=prefix, prefix_len=lens, return_logp=True))
    assert t.shape[1] == n                                            # no eos: the shortest prefix's row gets max_len columns
    for b, L in enumerate(lens):
        k = n - (L - 1)                                               # the row's first k columns are positions L-1 .. n-1 of the plain decode
        assert torch.equal(t[b, :k], toks[b, L - 1:]), (b, L)
        assert torch.equal(lp[b, :k], logp[b, L - 1:]), (b, L, float((lp[b, :k] - logp[b, L - 1:]).abs().max()))
        assert torch.equal(plp[b, 1:L], logp[b, :L - 1]), (b, L)      # the forced tokens were the arg-max: the same float
        assert bool((plp[b, 0] == 0) and (plp[b, L:] == 0).all())
    return toks, logp


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("dims", [W128, W128_ODD], ids=["v200", "v201"])
def test_forcing_the_models_own_tokens_changes_nothing(dims, dtype):
    d, sd, m = build(dims, seed=3, dtype=dtype, max_batch=8)
    m.eos_token = None
    img = _rgb(5, 41).cuda()
    _forced_identity(m, d, img, 12, [1, 7, 3, 12, 2])


def test_forced_identity_on_two_row_ranges_and_captured_steps():
    d, sd, m = build(W128, seed=3, dtype="bf16", max_batch=40)
    m.eos_token = None
    img = _rgb(40, 43, 32, 48).cuda()
    lens = [1 + (i * 5) % 9 for i in range(40)]
    _forced_identity(m, d, img, 10, lens, TXO_LANES=2)
    assert m._engine.query(Q_LAST_ROW_RANGES) == 2
    # B = 3: captured steps.  A second call with another prefix in the same engine replays the step with the NEW table
    d, sd, m = build(W128, seed=3, max_batch=3)
    m.eos_token = None
    img = _rgb(3, 44).cuda()
    toks, _ = _forced_identity(m, d, img, 12, [1, 5, 3], TXO_GRAPH=1)
    other = toks[:, :4].clone()
    other[:, 3] = (other[:, 3] + 1) % (d.vocab - 3)                   # a token the model did not pick
    prefix = torch.cat([torch.full((3, 1), d.bos, dtype=torch.int64, device="cuda"), other], 1)
    with knobs(TXO_GRAPH=1):
        a = _launch(m, lambda: m.generate(img, 6, prefix=prefix))
    with knobs(TXO_GRAPH=0):
        b = _launch(m, lambda: m.generate(img, 6, prefix=prefix))
    assert torch.equal(a, b) and not torch.equal(a, toks[:, 4:10])


# ---- 3. per-row lengths against float64 -----------------------------------------------------------------------------------------------
LENS = (1, 4, 9, 9, 2)


def _f64_case():
    """w128, lengths LENS, max_len 8: the first weight seed at which every free position's float64 top-2 margin is >= 1e-4"""
    d = W128
    img = _rgb(5, 47)
    rng = np.random.default_rng(5)
    prefix = torch.from_numpy(rng.integers(0, d.vocab - 3, (5, 9))).long()
    prefix[:, 0] = d.bos
    for seed in range(3, 12):
        sd = synth.synth_state_dict(d, seed)
        ref = prefix_ref.generate_prefix(ref64.sd64(sd), img.double(), prefix, LENS, None, 8, d.pad, bos=d.bos)
        if float(ref.margin.min()) >= 1e-4:
            return d, sd, img, prefix, ref
    raise AssertionError("no seed with a margin >= 1e-4 at every free position")


@pytest.fixture(scope="module")
def f64_case():
    return _f64_case()


def test_per_row_lengths_match_float64_fp32(f64_case):
    d, sd, img, prefix, ref = f64_case
    assert float(ref.margin.min()) >= 1e-4 and ref.tokens.shape == (5, 8)            # every position of every row: none left out
    _, _, m = build(d, sd=sd, max_batch=8)
    m.eos_token = None
    t, lp, plp = _launch(m, lambda: m.generate(img.cuda(), 8, prefix=prefix.cuda(), prefix_len=LENS, return_logp=True))
    assert torch.equal(t.cpu(), ref.tokens)
    junk = prefix.clone()                                             # columns at and behind a row's length are never read, nor checked
    for b, L in enumerate(LENS):
        junk[b, L:] = -1
    assert torch.equal(_launch(m, lambda: m.generate(img.cuda(), 8, prefix=junk.cuda(), prefix_len=LENS)), t)
    with pytest.raises(IndexError):
        m.generate(img.cuda(), 8, prefix=junk.cuda(), prefix_len=[2] + list(LENS[1:]))
    e1, e2 = float((lp.cpu().double() - ref.logp).abs().max()), float((plp.cpu().double() - ref.prefix_logp).abs().max())
    print(f"prompted decode vs float64, fp32: max |dlogp| {e1:.3e}, max |dprefix_logp| {e2:.3e}")
    assert e1 < FP32_LOGP and e2 < FP32_LOGP
    mn = min(LENS)
    for b, L in enumerate(LENS):
        assert bool((plp[b, :mn] == 0).all()) and bool((plp[b, L:] == 0).all()), b
        assert bool((plp[b, mn:L] < 0).all()), b
    # model.score() on the same sequences: prefix_logp and logp are its logp (position i-1 scores token i)
    for b, L in enumerate(LENS):
        seq = torch.cat([prefix[b, :L].cuda(), t[b]])[None]
        s = m.score(img[b:b + 1].cuda(), seq, mask=torch.ones_like(seq, dtype=torch.bool)).logp[0]
        assert float((s[L - 1:] - lp[b]).abs().max()) < 2 * FP32_LOGP, b
        if L > mn:
            assert float((s[mn - 1:L - 1] - plp[b, mn:L]).abs().max()) < 2 * FP32_LOGP, b


def test_per_row_lengths_match_float64_bf16(f64_case):
    """bf16 picks its own tokens: log-probabilities against float64 teacher-forced on the engine's tokens"""
    d, sd, img, prefix, _ = f64_case
    _, _, m = build(d, sd=sd, dtype="bf16", max_batch=8)
    m.eos_token = None
    t, lp, plp = _launch(m, lambda: m.generate(img.cuda(), 8, prefix=prefix.cuda(), prefix_len=LENS, return_logp=True))
    sd64 = ref64.sd64(sd)
    bound = 2 * BF16_BOUND["logits"]
    worst = 0.0
    for b, L in enumerate(LENS):
        seq = torch.cat([prefix[b, :L], t[b].cpu()])[None]
        lsm = torch.log_softmax(ref64.decoder_net(sd64, seq[:, :-1], ref64.encode(sd64, img[b:b + 1])), -1)[0]
        want = lsm.gather(1, seq[0, 1:, None])[:, 0]                  # want[i - 1] scores token i
        worst = max(worst, float((want[L - 1:] - lp[b].cpu().double()).abs().max()))
        if L > min(LENS):
            worst = max(worst, float((want[min(LENS) - 1:L - 1] - plp[b, min(LENS):L].cpu().double()).abs().max()))
        assert bool((plp[b, :min(LENS)] == 0).all()) and bool((plp[b, L:] == 0).all()), b
    print(f"prompted decode vs float64 teacher-forced, bf16: max |dlogp| {worst:.4f} (bound {bound:.4f})")
    assert worst < bound


# ---- 4. eos -----------------------------------------------------------------------------------------------------------------------------
def test_prefix_that_holds_eos_and_unreached_columns(f64_case):
    d, sd, img, prefix, ref = f64_case
    _, _, m = build(d, sd=sd, max_batch=8)
    sd64 = ref64.sd64(sd)
    # eos = a token row 0 (length 1) first picks in its column c >= 1; rows 1..4 hold it in their prefixes (row 2 at a position the loop has
    # yet to force)
    c = next(j for j in range(1, 8) if int(ref.tokens[0, j]) not in ref.tokens[0, :j].tolist())
    eos = int(ref.tokens[0, c])
    p = prefix.clone()
    p[p == eos] = (eos + 1) % (d.vocab - 3)
    p[:, 0] = d.bos
    p[1, 2] = p[2, 7] = p[3, 1] = p[4, 1] = eos
    m.eos_token = eos
    for stop in ("global", "row"):
        want = prefix_ref.generate_prefix(sd64, img.double(), p, LENS, eos, 8, d.pad, stop=stop, bos=d.bos)
        assert want.t_last == c and want.tokens.shape == (5, c + 1)  # the break is row 0's eos
        assert float(want.margin.min()) >= 1e-4
        with knobs(TXO_DEBUG_POISON=1):
            t, lp, plp = _launch(m, lambda: m.generate(img.cuda(), 8, prefix=p.cuda(), prefix_len=LENS, return_logp=True, stop=stop))
        assert torch.equal(t.cpu(), want.tokens), stop
        assert float((lp.cpu().double() - want.logp).abs().max()) < FP32_LOGP, stop
        # the forced tokens' log-probabilities: scored up to the break under the global stop (row 2's, at columns 1 .. c + 1); under the
        # per-row stop rows 1..4 are finished from the start and nothing is scored for them -- exactly 0.0
        assert float((plp.cpu().double() - want.prefix_logp).abs().max()) < FP32_LOGP, stop
        assert bool((plp[:, c + 2:] == 0).all()) and bool((plp[0] == 0).all())
        if stop == "global":
            assert bool((plp[2, 1:c + 2] < 0).all()) and bool((want.prefix_logp[2, 1:c + 2] < 0).all())
        else:
            assert bool((plp == 0).all()) and bool((want.prefix_logp == 0).all())
        assert bool((t[2:4] == d.pad).all()) and bool((lp[2:4] == 0).all())          # rows 2, 3 (length 9) never got behind their prefix
        if stop == "row":
            assert bool((t[1:] == d.pad).all()) and bool((lp[1:] == 0).all())        # a prefix that holds eos: all pad, 0.0
    # decoder.generate(stop='row', pad=): a caller's pad id takes the place of the engine's, as on the stepwise route
    enc = m.encoder(img.cuda())
    want7 = prefix_ref.generate_prefix(sd64, img.double(), p, LENS, eos, 8, 7, stop="row", bos=d.bos).tokens
    got7 = _launch(m, lambda: m.decoder.generate(p.cuda(), eos, 8, enc=enc, prefix_len=LENS, stop="row", pad=7))
    assert torch.equal(got7.cpu(), want7) and bool((got7[1:] == 7).all())
    # every row finished from the start: one position is decoded, one column comes back
    p[0, 0] = eos
    t = _launch(m, lambda: m.generate(img.cuda(), 8, prefix=p.cuda(), prefix_len=LENS))
    assert t.shape == (5, 1) and bool((t[1:] == d.pad).all())         # (no other row is behind its prefix at position 0)


def _first_compaction(lens, fin_pos, ranges, graph):
    """The position behind which the engine first compacts, from its schedule (engine.hip: generate_impl): a range's finished-row count is
    requested behind a position r with (r + 1) % TXO_STOP_EVERY == 0, read DonePoll::AHEAD = 4 positions later, and the range is compacted
    there if that frees TXO_STOP_GAIN rows (captured steps: in multiples of 16 rows); else the next request goes out at once.
    fin_pos[b]: the position at which row b holds eos (-1: from the start, None: never).  ranges: (first row, rows)."""
    every, gain, ahead = int(STOP_ENV["TXO_STOP_EVERY"]), int(STOP_ENV["TXO_STOP_GAIN"]), 4
    r = next(t for t in range(min(lens) - 1, 100) if (t + 1) % every == 0)
    while r < 100:
        for b0, nb in ranges:
            bound = nb - sum(1 for b in range(b0, b0 + nb) if fin_pos[b] is not None and fin_pos[b] <= r)
            if graph:
                bound = min(nb, (bound + 15) & ~15)
            if bound >= 1 and nb - bound >= gain:
                return r + ahead
        r += ahead
    return None


@pytest.mark.parametrize("lo", [1, 3], ids=["m1", "m3"])
@pytest.mark.parametrize("graph,lanes", [(0, 2), (1, 1)], ids=["eager_2ranges", "captured_1range"])
def test_row_stop_compactions_move_rows_in_their_forced_phase(graph, lanes, lo):
    """gpu_harness.stop_case (40 rows that finish anywhere between position 0 and never), every row prompted with the first len_b - 1 tokens
    it picks itself (lengths lo .. lo + 11: with lo = 3 the loop starts behind a multi-position pass), compactions every other position:
    rows are moved while they are still being forced, and every row's tokens up to its first eos are the uncompacted call's bit for bit.
    Eager launches on two row ranges (32 + 8 rows), captured steps on one (40 rows step down to 32: on two ranges no multiple of 16 is
    reached before position 38)."""
    d, sd, img = stop_case()
    _, _, m = build(d, sd=sd, max_batch=40, env=dict(STOP_ENV, TXO_STOP_GRAPH=str(graph)))
    x = img.cuda()
    with knobs(TXO_LANES=lanes):
        base = _launch(m, lambda: m.generate(x, d.max_len))
    lens = [lo + (i * 7) % 12 for i in range(40)]
    n = d.max_len - (max(lens) - 1)                                   # the loop runs over the whole table: the finishing schedule of stop_case
    prefix = torch.cat([torch.full((40, 1), d.bos, dtype=torch.int64, device="cuda"), base[:, :max(lens) - 1]], 1)
    # the schedule: the first compaction comes while rows that it moves (live, behind a finished row of their range) are still being forced
    bf = first_eos(base.cpu().numpy(), d.eos)
    fin_pos = [-1 if d.eos in prefix[b, :L].tolist() else (None if bf[b] < 0 else bf[b]) for b, L in enumerate(lens)]
    ranges = [(0, 32), (32, 8)] if lanes == 2 else [(0, 40)]
    first = _first_compaction(lens, fin_pos, ranges, graph)
    assert first is not None and first < max(lens) - 1, first
    live = lambda b: fin_pos[b] is None or fin_pos[b] > first
    forced_and_moved = [b for b0, nb in ranges for b in range(b0, b0 + nb)
                        if live(b) and lens[b] - 1 > first and any(not live(q) for q in range(b0, b))]
    assert len(forced_and_moved) >= 3, forced_and_moved
    with knobs(TXO_LANES=lanes):
        glob = _launch(m, lambda: m.generate(x, n, prefix=prefix, prefix_len=lens))
        assert m._engine.query(Q_LAST_COMPACTIONS) == 0
        row, lp, _ = _launch(m, lambda: m.generate(x, n, prefix=prefix, prefix_len=lens, stop="row", return_logp=True))
    assert m._engine.query(Q_LAST_COMPACTIONS) > 0 and m._engine.query(Q_LAST_ROW_RANGES) == lanes
    assert row.shape == glob.shape
    g, r = glob.cpu().numpy(), row.cpu().numpy()
    for b, L in enumerate(lens):
        if fin_pos[b] == -1:
            assert (r[b] == d.pad).all() and bool((lp[b] == 0).all()), b
            continue
        f = first_eos(g[b:b + 1], d.eos)[0]
        upto = g.shape[1] if f < 0 else f + 1
        assert np.array_equal(r[b, :upto], g[b, :upto]), (b, L)
        assert (r[b, upto:] == d.pad).all() and bool((lp[b, upto:] == 0).all()), b
        k = min(upto, base.shape[1] - (L - 1))
        assert np.array_equal(r[b, :k], base[b, L - 1:L - 1 + k].cpu().numpy()), (b, L)      # and the plain decode's, shifted by the row's prefix
        assert f < 0 or f + L - 1 == fin_pos[b], (b, L)               # (the schedule above was the decode's)


# ---- 5. forms, ragged batches, the decode path ----------------------------------------------------------------------------------------
def test_latent_cross_form_equals_the_kv_form():
    d64 = SHAPE_CASES["w64_h4"][0]                                    # the latent tile exists at width 64
    img = _rgb(5, 47)
    rng = np.random.default_rng(6)
    prefix = torch.from_numpy(rng.integers(0, d64.vocab - 3, (5, 9))).long()
    prefix[:, 0] = d64.bos
    lens_sets = (LENS, (3, 4, 9, 9, 5))                               # m == 1, and m == 3: the multi-position pass in front of the latent loop
    sd = refs = None
    for seed in range(3, 12):
        sd = synth.synth_state_dict(d64, seed)
        refs = [prefix_ref.generate_prefix(ref64.sd64(sd), img.double(), prefix, ls, None, 8, d64.pad, bos=d64.bos) for ls in lens_sets]
        if min(float(r.margin.min()) for r in refs) >= 1e-4:
            break
    assert min(float(r.margin.min()) for r in refs) >= 1e-4
    for latent in (0, 1):
        _, _, m = build(d64, sd=sd, max_batch=8, latent=latent)
        m.eos_token = None
        for ls, ref in zip(lens_sets, refs):
            t, lp, plp = m.generate(img.cuda(), 8, prefix=prefix.cuda(), prefix_len=ls, return_logp=True)
            assert m._engine.query(Q_LAST_LATENT) == latent and m._engine.query(Q_LAST_PERSISTENT) == 0
            assert torch.equal(t.cpu(), ref.tokens), (latent, ls)
            assert float((lp.cpu().double() - ref.logp).abs().max()) < FP32_LOGP, (latent, ls)
            assert float((plp.cpu().double() - ref.prefix_logp).abs().max()) < FP32_LOGP, (latent, ls)


def test_multi_position_pass_in_front_of_two_row_ranges():
    """m = 3 at 40 rows in fp32 (a row's bits do not depend on the batch or its ranges): two row ranges behind the multi-position pass
    return what one range returns, bit for bit"""
    d, sd, m = build(W128, seed=3, max_batch=40)
    m.eos_token = None
    img = _rgb(40, 43, 32, 48).cuda()
    toks = _launch(m, lambda: m.generate(img, 12))
    lens = [3 + (i * 5) % 9 for i in range(40)]
    prefix = torch.cat([torch.full((40, 1), d.bos, dtype=torch.int64, device="cuda"), toks[:, :max(lens) - 1]], 1)
    out = {}
    for lanes in (1, 2):
        with knobs(TXO_LANES=lanes):
            out[lanes] = _launch(m, lambda: m.generate(img, 10, prefix=prefix, prefix_len=lens, return_logp=True))
        assert m._engine.query(Q_LAST_ROW_RANGES) == lanes
    for a, b in zip(out[1], out[2]):
        assert torch.equal(a, b)
    for b, L in enumerate(lens):                                      # and the tokens are the plain decode's, shifted by the row's prefix
        k = 12 - (L - 1)
        assert torch.equal(out[2][0][b, :k], toks[b, L - 1:]), (b, L)
        assert bool((out[2][2][b, 3:L] < 0).all()) and bool((out[2][2][b, :3] == 0).all()) and bool((out[2][2][b, L:] == 0).all()), b


def test_ragged_prompted_rows_equal_the_solo_calls():
    d, sd, m = build(W128, seed=3, max_batch=len(TINY_SIZES))
    imgs = [torch.from_numpy(synth.synth_images(1, 3, h, w, seed=200 + i))[0].cuda() for i, (h, w) in enumerate(TINY_SIZES)]
    B = len(imgs)
    rng = np.random.default_rng(8)
    prefix = torch.from_numpy(rng.integers(0, d.vocab - 3, (B, 6))).long().cuda()
    prefix[:, 0] = d.bos
    lens = [2, 6, 3, 2, 5, 4, 6]
    m.eos_token = None
    t, lp, plp = m.generate_ragged(imgs, 9, prefix=prefix, prefix_len=lens, return_logp=True)
    assert m._engine.query(Q_LAST_PERSISTENT) == 0 and t.shape == (B, 9)
    for b in range(B):
        # the solo call with the batch's m: a second row of length min(lens) on the same image keeps the start of the loop where the batch's is
        two = prefix[[b, b]]
        t1, lp1, plp1 = m.generate(imgs[b][None].expand(2, -1, -1, -1).contiguous(), 9, prefix=two, prefix_len=[lens[b], min(lens)], return_logp=True)
        assert torch.equal(t[b], t1[0]) and torch.equal(lp[b], lp1[0]) and torch.equal(plp[b], plp1[0]), (b, TINY_SIZES[b])


def test_prompted_calls_leave_the_default_path_alone():
    """a 256-wide decoder (the persistent launch exists for it): plain generate() is persistent and bit-identical before and behind a
    prompted call, which never is"""
    d = SHAPE_CASES["calib256"][0]
    _, _, m = build(d, seed=2, dtype="bf16", max_batch=8)
    m.eos_token = None
    img = _rgb(4, 51).cuda()
    before = m.generate(img, 10, return_logp=True)
    assert m._engine.query(Q_LAST_PERSISTENT) == 1
    prefix = torch.cat([torch.full((4, 1), d.bos, dtype=torch.int64, device="cuda"), before[0][:, :4]], 1)
    t = m.generate(img, 6, prefix=prefix, prefix_len=[5, 1, 3, 5])
    assert m._engine.query(Q_LAST_PERSISTENT) == 0 and t.shape == (4, 6)
    after = m.generate(img, 10, return_logp=True)
    assert m._engine.query(Q_LAST_PERSISTENT) == 1
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


def test_a_step_behind_a_prompted_call_picks_for_itself():
    """the session a prompted call leaves is an ordinary one: txo_decode_step behind it returns the arg-max of its own logits -- what it
    returns behind txo_decode_begin --, not a token of the finished call's prefix"""
    meta, g = load_golden("ragged_prefix")
    d, sd, m = build(meta, max_batch=3)
    eng = m._engine
    m.eos_token = None
    img = images(meta).cuda()
    enc = m.encoder(img)
    start = torch.from_numpy(g["start"].astype(np.int64)).cuda()
    bos = torch.full((3,), d.bos, dtype=torch.int64, device="cuda")
    eng.decode_begin(enc)
    l0, t0 = eng.decode_step(0, bos)
    l1, t1 = eng.decode_step(1, t0)
    assert bool((start[:, 1] != t0).any())                            # (the prefix would force another token at position 0)
    T0 = start.shape[1]
    for call in (lambda: m.decoder.generate(start, None, 4, enc=enc, prefix_len=[T0, 2, 3]),
                 lambda: m.generate(img, 4, prefix=start, prefix_len=[2, T0, T0], return_logp=True),
                 lambda: m.generate(img, 4, prefix=start, decode="sample", seed=5)):
        call()
        a0, b0 = eng.decode_step(0, bos)
        a1, b1 = eng.decode_step(1, b0)
        assert torch.equal(b0, t0) and torch.equal(a0, l0) and torch.equal(b1, t1) and torch.equal(a1, l1)
        assert torch.equal(b0, l0.argmax(-1))


# ---- 6. facades and refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_session_alone():
    meta, g = load_golden("ragged_prefix")
    d, sd, m = build(meta, max_batch=3)
    eng = m._engine
    img = images(meta).cuda()
    enc = m.encoder(img)
    start = torch.from_numpy(g["start"].astype(np.int64)).cuda()
    eng.decode_begin(enc)
    logits0, tok0 = eng.decode_step(0, start[:, 0].contiguous())
    ses = eng.session

    def still_open():
        assert eng.session is ses
        l, t = eng.decode_step(0, start[:, 0].contiguous())
        assert torch.equal(l, logits0) and torch.equal(t, tok0)

    T = d.max_len
    for kw, frag in ((dict(prefix=start, max_len=T), "longest prefix"), (dict(prefix=start, prefix_len=[0, 1, 1], max_len=4), "prefix_len must be in"),
                     (dict(prefix=start, prefix_len=[1, 1], max_len=4), "one entry per row"), (dict(prefix=start[:2], max_len=4), "prefix must be"),
                     (dict(prefix=start, max_len=4, beam=2), "prefix= is not available with beam"),
                     (dict(prefix=start, max_len=4, return_logits=True), "prefix= is not available with return_logits")):
        with pytest.raises(ValueError, match=frag):
            m.generate(img, **kw)
        still_open()
    with pytest.raises(IndexError):
        m.generate(img, 4, prefix=torch.full_like(start, d.vocab))
    still_open()
    # the C ABI refuses the same before anything is encoded (the session's K/V history would change): TXO_E_INVALID, messages name the prefix
    for lens, n, frag in (([0, 1, 1], 4, "prefix_len[0]"), ([1, 1, start.shape[1] + 1], 4, "prefix_len[2]"), (None, T, "longest prefix")):
        rc, *_ = _abi_from_enc(eng, enc, start, n, -1, lens)
        assert rc == -1 and "prefix" in eng.lib.txo_last_error().decode() and frag in eng.lib.txo_last_error().decode()
        still_open()
    # beyond the table / with a padding mask decoder.generate keeps the stepwise loop, and return_logp keeps its refusal there
    with pytest.raises(ValueError, match="return_logp needs"):
        m.decoder.generate(start, None, T, enc=enc, return_logp=True)
    assert m.decoder.generate(start, None, T, enc=enc).shape == (3, T)


def test_wrapper_continues_a_latex_prefix(tmp_path):
    from PIL import Image
    from texocr_amd.config import default_config
    from texocr_amd.tokenizer import RegExTokenizer, process_output
    from texocr_amd.wrapper import TeXOCRWrapper
    v = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tokenizer_vocab_1k.json")))
    RegExTokenizer.from_tables(v["vocab_size"], v["special_tokens"], v["merges"]).save(str(tmp_path / "vocab.txt"))
    cfg = default_config(img_size=[64, 256], max_length=32, in_channels=1,
                         encoder={"embed_dim": 64, "heads": 2, "num_layers": 1}, decoder={"embed_dim": 64, "heads": 2, "num_layers": 2})
    cfg["tokenizer_path"] = str(tmp_path / "vocab.txt")
    w = TeXOCRWrapper(cfg, max_batch=3)
    w.model.load_state_dict(synth.synth_state_dict(w.dims, 5))
    rng = np.random.RandomState(0)
    pil = []
    for wd, ht in [(200, 40), (30, 30), (250, 64), (100, 17)]:
        a = np.full((ht, wd, 3), 255, dtype=np.uint8)
        a[rng.randint(0, ht, 40), rng.randint(0, wd, 40)] = rng.randint(0, 120, (40, 1))
        pil.append(Image.fromarray(a))
    text = r"\begin{aligned} x"
    ids = w.tokenizer.encode(text)
    plain = w(pil[0], max_len=12, decode="greedy")
    # forcing the model's own first tokens gives the rest of the plain decode, and the LaTeX of the whole
    own = w(pil[0], max_len=9, decode="greedy", prefix=plain[0][:3])
    assert own[0] == plain[0][3:] and own[1] == plain[1]
    toks, latex, logp = w(pil[0], max_len=12, decode="greedy", prefix=text, return_logp=True)
    assert latex == process_output(w.tokenizer.decode(ids + toks)) and latex.startswith(process_output(text)[:6])
    assert len(logp) == len(toks) and all(x <= 0.0 for x in logp)
    assert w(pil[0], max_len=12, decode="greedy", prefix=ids)[:2] == (toks, latex)     # a token list is the string's tokens
    # batch: one prefix per image, strings and token lists, equal to the per-image calls
    pres = [text, ids[:2], "x", plain[0][:3]]
    got = w.batch(pil, max_len=12, decode="greedy", prefix=pres)
    for b, (im, p) in enumerate(zip(pil, pres)):
        assert got[b] == w(im, max_len=12, decode="greedy", prefix=p), b
    with pytest.raises(ValueError, match="one entry per image"):
        w.batch(pil, prefix=[text])
    with pytest.raises(ValueError, match="prefix= is not available with decode='beam'"):
        w(pil[0], decode="beam", prefix=text)
    with pytest.raises(ValueError, match="no room"):
        w(pil[0], prefix=list(range(1, 40)))
